// mg_types.inc - part of libmgvcycle.so's single translation unit (included by mgvcycle.hip in this order; not compiled on its own).
// Options (switches read once per handle), device buffers, the operator (Csr) with every device format it may carry, levels, the hierarchy handle.
namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

// Busy-poll instead of hipStreamSynchronize: one 8-byte readback per step sits on the critical path of the
// solve loop, so the thread spins on hipStreamQuery rather than parking on an interrupt.
static inline hipError_t spin_sync(hipStream_t s) {
  hipError_t e;
  while ((e = hipStreamQuery(s)) == hipErrorNotReady) {
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
  return e;
}

// x == 0 everywhere?  Blocks of 4096 entries are OR-reduced bitwise (vectorises; the element-wise loop with its early
// exit does not: 13 ms for 136 MB on the box's core) and only a block with a set bit - a non-zero or a -0.0 - is
// looked at entry by entry.
bool host_all_zero(const double* x, long long len) {
  const long long B = 4096;
  for (long long i0 = 0; i0 < len; i0 += B) {
    const long long i1 = std::min(len, i0 + B);
    unsigned long long acc = 0;
    for (long long i = i0; i < i1; ++i) {
      unsigned long long bits;
      std::memcpy(&bits, x + i, 8);
      acc |= bits;
    }
    if (acc != 0)
      for (long long i = i0; i < i1; ++i)
        if (x[i] != 0.0) return false;
  }
  return true;
}

// Switches and thresholds of the format selection (A/B measurements, tests).  Read from the environment ONCE per
// handle - at mg_create / mg_op_create - and kept in the handle; mg_set_option overrides single entries through the
// API before the operators are uploaded.  Nothing on the launch path reads the environment.
// One line per option, X(type, key, default): the field, the key mg_set_option takes and, in upper case behind "MG_",
// the environment variable (no_tile: MG_NO_TILE).
#define MG_OPTIONS(X) \
  X(bool, no_rowclass, false) \
  X(bool, no_implicit_first, false) \
  X(bool, no_class_d, false) \
  X(bool, no_tile, false) \
  X(bool, no_window, false) \
  X(bool, no_pattern, false) \
  X(bool, no_runs, false) \
  X(bool, no_sched, false) \
  X(bool, no_pair, false) \
  X(bool, no_fused_next, false) \
  X(bool, no_march, false) \
  X(bool, no_lane, false) \
  X(bool, no_lane_mm, false) \
  X(bool, no_tile_small, false) \
  X(bool, no_march2, false)        /* never fuse a sweep with the residual that follows it (csr_rowclass_march2_spmv) */ \
  X(bool, no_tile_lane, false) \
  X(bool, no_winp, false) \
  X(bool, no_band, false) \
  X(bool, no_lane_rpl3, false) \
  X(bool, no_march2_zero, false) \
  X(bool, no_mgs_chain, false) \
  X(bool, no_restrict_scale, false) \
  X(long long, rap_chunk, 2048)    /* target columns of a coarse row the numeric Galerkin product accumulates at a time (<= 2048; tests) */ \
  X(long long, rap_groups, 0)      /* CF64 numeric Galerkin product: rows of A walked side by side by a wavefront (0: default; 1, 2, 4, 8, 16; A/B, tests) */ \
  X(bool, no_dead_t, false)        /* solve loop: store the iterate of every step (A/B, bit-identity tests) */ \
  X(bool, no_march3, false)        /* never use the 2-D tile form of the two-stage pass (csr_rowclass_march3_spmv) */ \
  X(long long, march3_k1, 0)       /* rows of the stage-1 region per lane (0: by the fill estimate; 2..4): tile height = K1 * (NT / (TX + 2)) - 2 */ \
  X(long long, march3_nt, 0)       /* threads per workgroup (0: by the fill estimate; 1024 or 768) */ \
  X(long long, march3_tiles_x, 0)  /* 0: chosen by the fill estimate; > 0: this many tiles per grid line */ \
  X(bool, no_march3_lockstep, false)      /* schedule of the 2-D tile form */ \
  X(bool, march3_lockstep_force, false)   /* schedule of the 2-D tile form */ \
  X(bool, no_pipeline, false)      /* solve loop: read a four-stage step's norm before the next step is enqueued (A/B) */ \
  X(bool, no_march4, false)        /* solve loop: never run the two fine-level passes across the stopping test as one four-stage pass */ \
  X(long long, march4_nt, 0)       /* threads per workgroup of the four-stage pass (0: default; 1024 / 768 / 512 = 2 / 3 / 4 rows per lane) */ \
  X(long long, march4_tiles_x, 0)  /* 0: chosen by the fill estimate; > 0: this many tiles per grid line */ \
  X(long long, march4_ty_max, 0)   /* tests: tallest tile (several tile rows on small grids) */ \
  X(long long, march4_segs, 0)     /* A/B, tests: segments per tile (0: chosen by the cost model; tiles x segments may exceed the CUs) */ \
  X(long long, columns_streams, 2) /* column-wise block solve: streams the columns take turns on (1: one stream; at most 8) */ \
  X(bool, no_columns, false)       /* blocks of right-hand sides: never solve column by column on the single-vector kernels (A/B) */ \
  X(bool, no_marchr, false)        /* restriction: the gather form (csr_rowclass_lane_spmv) on every level (A/B) */ \
  X(long long, marchr_min_rows, 1000000)   /* coarse rows below which the gather form stays */ \
  X(long long, marchr_segs, 0)     /* A/B, tests */ \
  X(long long, marchr_tx, 0)       /* A/B, tests */ \
  X(long long, marchr_ty, 0)       /* A/B, tests */ \
  X(bool, no_march27, false)       /* 27-point levels: plane-tile kernel, sweep and residual as two launches (A/B) */ \
  X(bool, no_defer_sum, false)     /* solve loop: the four-stage pass's final sum as a launch of its own instead of one more workgroup of the fine restriction (A/B) */ \
  X(bool, no_small_fuse, false)    /* small levels: residual + restriction and prolongation + first post-sweep as two launches each (round 5's path; A/B) */ \
  X(bool, no_march27_zero, false)  /* the 27-point pair of a level entered with x = 0 reads x1 = d.*b written by the restriction (round 5's path; A/B) */ \
  X(long long, march27_nt, 0)      /* A/B, tests (0: chosen by the cost model) */ \
  X(long long, march27_tiles_x, 0) /* A/B, tests (0: chosen by the cost model) */ \
  X(long long, march27_segs, 0)    /* A/B, tests (0: chosen by the cost model) */ \
  X(long long, march27_wgs, 0)     /* A/B, tests (0: chosen by the cost model) */ \
  X(long long, march27_min_rows, 500000)   /* smaller levels are latency-bound: the 256-row plane tiles serve them */ \
  X(long long, march4_k1, 0)       /* rows per lane (0: 2 / 3 / 4 at 1024 / 768 / 512 threads; 768 threads also take 4) */ \
  X(bool, no_small, false)         /* small grid levels: never use the one-trip kernels of mg_small.hpp (A/B) */ \
  X(long long, small_max_rows, 300000)     /* largest level (rows of A / coarse rows of R / fine rows of P) they serve */ \
  X(bool, no_band27, false)        /* variable-coefficient 27-point grid levels: pattern-coded CSR kernels instead of the planar band-27 form (A/B) */ \
  X(long long, band27_max_rows, 40000000)  /* largest operator held in band-27 form (216 B per row on top of the CSR arrays) */ \
  X(bool, no_ci16, false)          /* long rows: keep 32-bit column indices (A/B) */ \
  X(bool, force_rowptr64, false)   /* upload every operator with 64-bit row pointers (the path of operators with >= 2^31 non-zeros; tests) */ \
  X(bool, no_longrow, false)       /* never use csr_longrow_spmv (one wavefront per row) for operators of long rows (A/B) */ \
  X(long long, longrow_min_avg, 1000)      /* ... it serves operators without row classes whose rows average at least this many entries */ \
  X(long long, small_p_max_rows, 4000000)  /* the arithmetic prolongation up to this many fine rows (C2: level 2 13.9 us against 19.0 for the staged \
                                              windows, level 1 85.5 against 86.8 - left on the windows; profiles/r05_small_levels.md) */ \
  X(long long, small_r_max_rows, 0)        /* A/B: the small restriction up to this many coarse rows (0: small_max_rows; 2.1 M rows: 64 us against 54 marching) */ \
  X(long long, small_over_rc, 0)   /* ... also where the operator is stored as row classes, up to this many rows (A/B; by default the \
                                      small kernels replace the STREAMING kernels of the levels below rowclass_min_rows) */ \
  X(bool, debug_format, false) \
  X(bool, debug_timing, false) \
  X(int, nt, -1)                   /* -1: by operator size; 0 / 1: force the cache policy of the matrix stream */ \
  X(long long, rowclass_min_rows, 100000) \
  X(long long, rowclass_max_passes, 4) \
  X(long long, rowclass_keep_singletons, 1024) \
  X(long long, stage_min_len, 1) \
  X(long long, tile_min_wg, 256) \
  X(long long, window_min_wg, 2048) \
  X(long long, pair_min_rows, 1000000) \
  X(long long, march_min_wg, 256) \
  X(long long, march_wg_per_cu, 2) /* resident workgroups per CU of the marching kernel (49 KB of LDS each) */ \
  X(long long, winp_min_rows, 100000)      /* smallest prolongation-shaped operator served by csr_rowclass_winp_spmv */ \
  X(bool, no_wave_restrict, false) /* restrictions of vertex-centred grid pairs: the marching / lane-per-row kernels instead of the wavefront form (A/B) */ \
  X(long long, wave_restrict_min_rows, 0) \
  X(bool, no_cell_prolong, false)  /* prolongations of vertex-centred grid pairs: the windowed / lane-per-row kernels instead of the lane-per-coarse-cell one (A/B) */ \
  X(bool, no_band_sym, false)      /* band form: read all 7 planes even where the operator is symmetric */ \
  X(bool, band_sym_tol, false)     /* band-27 levels: accept symmetry up to the rounding of the Galerkin product (2^-50 |a_ii|) for the symmetric reads - \
                                      the operator applied then differs from the stored CSR at rounding level (default: bit-for-bit symmetry only) */ \
  X(long long, band_min_rows, 100000)      /* smallest variable-coefficient grid operator held in band form (build_band) */ \
  X(long long, march_max_len, 8)   /* longest class the marching kernel is used for (27-point levels: plane tiles, measured) */ \
  X(bool, dist_tail_graph, false)  /* replay the replicated tail of the sharded sequencer as a HIP graph (measured slower) */ \
  X(bool, no_graph, false) \
  X(bool, no_lane_pairs, false) \
  X(long long, graph_max_rows, 300000)     /* sub-cycles from the first level of at most this many rows*nrhs replay as one HIP graph */ \
  X(long long, lu_multi_min_rows, 4096)    /* sparse coarse factors of this many rows: per-level launches + dense trailing inverse */ \
  X(long long, coarse_gmres_tail_rows, -1) /* complex GMRES coarsest solve: largest level whose steps run the one-workgroup tail (-1: the measured \
                                              default; 0: the chain of passes everywhere; capped by the tail's row limit; read at every solve). \
                                              TWO UNITS: the single-vector solve compares it with the coarsest ROWS n_c, the block solve \
                                              (coarse_gmres_blocks) with the block's VALUES n_c * nrhs - one number moves both thresholds */ \
  X(bool, coarse_gmres_blocks, false)      /* complex GMRES coarsest solve: serve blocks of right-hand sides by the block form of the solve \
                                              (blockFGMRES, cx_coarse_block_gmres); 0: a block on such a hierarchy is refused; read at every call */ \
  X(bool, vanka_blocks, false)             /* complex Vanka hierarchies (relaxation type 2): serve blocks of right-hand sides by the block \
                                              form of the smoother (the _blk kernels of mg_vanka.hpp); 0: a block on such a hierarchy is \
                                              refused; read at every call */ \
  X(bool, single_kcycle, false)            /* ComplexF32 hierarchies: serve the K-cycle and Jac-GMRES smoothing (mg_set_schedule_CF32, \
                                              mg_fgmres_relax_CF32; Gram sums and least squares in double); 0: refused on a CF32 \
                                              handle, as before the single form existed; read at mg_finalize and at every call */ \
  X(bool, kcycle_blocks, false)            /* complex hierarchies with cycle 'K' and / or Jac-GMRES smoothing: serve blocks of right-hand \
                                              sides by the reference's long-vector form (one H, xi, t and break test per relaxation for \
                                              the whole block: the columns are coupled; the GRAM mode of cx_csr_stream_spmm); 0: a \
                                              block on such a hierarchy is refused, as before that form existed; set before \
                                              mg_finalize, read at every call */ \
  X(bool, vanka_device_setup, false)       /* complex Vanka hierarchies whose blocks were built on the device (mg_build_vanka_CF64): \
                                              mg_rap_CF64 recomputes the operators and rebuilds the blocks in HBM; 0: it refuses a \
                                              Vanka handle, as before the device build existed; read at every call */ \
  X(bool, coarse_device_inverse, false)     /* the explicit inverse of the coarsest operator is built in HBM (mg_build_coarse_dense_inverse_*): \
                                              mg_rap_FP64 / mg_rap_CF64 rebuild it behind the last Galerkin product while the coarsest solve is \
                                              a dense inverse; 0: they leave it to the host, as before the device build existed; read at every call */ \
  X(long long, coarse_device_inverse_max, 8192)   /* largest order the device build serves (at most 8192: work matrix plus result 2 x 1.07 GB complex) */ \
  X(long long, lu_dense_tail_min, 64) \
  X(long long, lu_dense_tail_max, 16384)   /* largest trailing block kept as an explicit inverse (8*M^2 bytes each for L and U: 2 x 2.1 GB) */ \
  X(double, rowclass_min_cover, 0.9) \
  X(double, sched_budget, 2.0e6)

struct Options {
#define MG_OPT_FIELD(type, key, def) type key = def;
  MG_OPTIONS(MG_OPT_FIELD)
#undef MG_OPT_FIELD
  bool set(const char* key, double v);   // false: no option of that key
  static Options from_env();
};
bool Options::set(const char* key, double v) {
#define MG_OPT_SET(type, k, def)   \
  if (std::strcmp(key, #k) == 0) { \
    k = static_cast<type>(v);      \
    return true;                   \
  }
  MG_OPTIONS(MG_OPT_SET)
#undef MG_OPT_SET
  return false;
}
// the environment variable of an option: "MG_" + the key in upper case
std::string option_env(const char* key) {
  std::string e = "MG_";
  for (const char* c = key; *c; ++c) e += (*c >= 'a' && *c <= 'z') ? (char)(*c - 'a' + 'A') : *c;
  return e;
}
// an option's value from its environment variable; historical semantics of the boolean switches: "1" switches on,
// anything else off
void env_value(bool& o, const char* e) { o = (e[0] == '1'); }
template <typename T>
void env_value(T& o, const char* e) { o = static_cast<T>(std::atof(e)); }
Options Options::from_env() {
  Options o;
#define MG_OPT_ENV(type, k, def) \
  if (const char* e = std::getenv(option_env(#k).c_str())) env_value(o.k, e);
  MG_OPTIONS(MG_OPT_ENV)
#undef MG_OPT_ENV
  if (std::getenv("MG_DEBUG_TIMING")) o.debug_timing = true;   // (any value)
  if (o.sched_budget < 1.0) o.sched_budget = 1.0;
  return o;
}

#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return fail(MG_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                  __LINE__);                                                                 \
  } while (0)

#define MG_TRY(expr)            \
  do {                          \
    int rc_ = (expr);           \
    if (rc_ != MG_OK) return rc_; \
  } while (0)

// The value type of a handle is fixed at creation (mg_create / mg_create_CF64): an FP64 entry point refuses a CF64 handle
// (MG_ERR_STATE), and the capabilities the CF64 path does not serve say so (MG_ERR_UNSUPPORTED).
#define MG_REAL_ONLY(h)                                                                                     \
  do {                                                                                                      \
    if ((h) && (h)->cx) return fail(MG_ERR_STATE, "%s: FP64 entry point called on a CF64 handle", __func__); \
  } while (0)
#define MG_CF64_UNSUPPORTED(h)                                                                              \
  do {                                                                                                      \
    if ((h) && (h)->cx) return fail(MG_ERR_UNSUPPORTED, "%s is not served for CF64 handles", __func__);    \
  } while (0)

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  int alloc(size_t count) {
    release();
    if (count == 0) count = 1;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T)));
    n = count;
    return MG_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  size_t bytes() const { return n * sizeof(T); }
};

struct Csr {
  Options opt;   // copied from the owning handle at upload
  bool set = false;
  long long n_rows = 0, n_cols = 0, nnz = 0;
  DevBuf<int> rowptr, colidx, blk_row, sched;
  DevBuf<int> blk_row_mm, sched_mm;  // second, smaller row-block partition for the block-RHS kernels
  std::vector<int> h_blk_row_mm;
  bool has_sched_mm = false;
  int nblocks_mm = 0;
  DevBuf<double> val;
  // pattern-coded column indices (csr_pattern_spmv): first column + pattern id per row, offset dictionary
  DevBuf<int> firstcol, pat_ptr, pat_off, run_ptr, runs;
  DevBuf<unsigned short> pat;
  bool has_runs = false;
  long long nruns_total = 0;
  bool has_pat = false;
  long long npat = 0, dict_entries = 0;
  // row classes (csr_rowclass_spmv): first column + class id per row, dictionary of (offset, value) rows
  DevBuf<int> rc_first, rc_ptr, rc_off, rc_delta, rw_meta, rw_lb, rt_lb, rc_exc;
  int rc_nexc = 0;          // exception rows (class id 0xFFFF), computed by csr_rows_spmv from the CSR arrays
  std::vector<int> h_rc_ptr, h_rc_off, h_rc_delta;   // host copy of the dictionary (tile index tables)
  int rc_major = 0;         // most frequent class
  bool rc_tile = false;     // csr_rowclass_tile_spmv (plane tiles from the grid hint)
  bool rc_march = false;    // csr_rowclass_march_spmv (z-marching ring of slabs; preferred over the tiles when set)
  DevBuf<int> rm_lb;
  int rm_P = 0, rm_nplanes = 0, rm_halo = 0, rm_chunks = 0, rm_nblocks = 0;
  bool rc_march2 = false;   // csr_rowclass_march2_spmv can serve a sweep + residual pair on this operator
  int rm2_nblocks = 0;
  bool rc_march3 = false;   // ... and so can csr_rowclass_march3_spmv (2-D in-plane tiles, z-star classes): preferred
  DevBuf<int> rc_exc2;      // box operators on the 2-D tile form: rows whose stage 2 is left to csr_rows_spmv (the layer behind the faces)
  int rc_nexc2 = 0;
  DevBuf<mgk::M3Class> rm3_cls;
  DevBuf<unsigned short> rm3_cmap;   // cx | cy | cz | tab: class id = tab[cz[z]][cy[y]][cx[x]]
  mgk::March3Dev rm3{};     // tile geometry
  size_t rm3_lds = 0;
  int rm3_k1 = 3, rm3_nt = 1024;
  double rm3_fill = 0.0;    // estimated L1 fills + stores per row (bytes) of the chosen geometry
  // four-stage pass of the solve loop (csr_rowclass_march4_spmv): same classes and product map, its own tile geometry
  bool rc_march4 = false;
  DevBuf<mgk::M4Class> rm4_cls;
  DevBuf<int> rm4_ysh;
  mgk::March4Dev rm4{};
  size_t rm4_lds = 0;
  int rm4_k1 = 3, rm4_nt = 768;
  double rm4_fill = 0.0;
  // 27-point grid operators (csr_rowclass_march27_spmv): canonical 27-value class records, the product map, one geometry for
  // the single product ([0]) and one for the sweep + residual pair ([1])
  bool rc_march27 = false;
  DevBuf<mgk::M27Class> rm27_cls;
  DevBuf<unsigned short> rm27_cmap;
  DevBuf<double> rm27_sink;
  mgk::March27Dev rm27[2]{};
  size_t rm27_lds[2] = {0, 0};
  int rm27_nt[2] = {0, 0}, rm27_pitch[2] = {0, 0};
  // marching restriction (csr_rowclass_marchr_spmv): R of a vertex-centred grid pair, canonical 27-value records over the coarse grid
  bool rc_marchr = false;
  DevBuf<mgk::M27Class> rmr_cls;
  DevBuf<unsigned short> rmr_cmap;
  mgk::MarchRDev rmr{};
  size_t rmr_lds = 0;
  // small grid levels (mg_small.hpp): position-code records of a 27-point operator / of a restriction over the coarse grid; the
  // prolongation form needs no table (full weighting, verified)
  bool sm_ok = false, smr_ok = false, smp_ok = false;
  bool waver_ok = false;           // R: verified scale * P' of the trilinear P (any size): grid_wave_restrict
  double waver_scale = 0.0;
  bool cellp_ok = false;           // P: verified trilinear interpolation of a vertex-centred grid pair of ANY size (smp holds its grids): grid_cell_prolong
  DevBuf<double> sm_rec, smr_rec;
  mgk::Small27Dev sm{};
  mgk::SmallRDev smr{};
  mgk::SmallPDev smp{};
  const double* sm_d_bound = nullptr;   // the relaxPrec vector the records' d was verified against
  // band-27 (grid27_band_spmv): 27 planar value arrays of a variable-coefficient 27-point grid operator
  bool b27_ok = false;
  DevBuf<double> b27_val;
  DevBuf<int> b27_flag;
  mgk::Band27Dev b27{};
  DevBuf<unsigned short> ci16;     // long rows: column index - the row's first column (when every row spans < 65536 columns)
  DevBuf<int> rowbase;             // ... and that first column per row
  bool has_ci16 = false;
  bool longrow() const { return !has_rc && !opt.no_longrow && n_rows > 0 && nnz >= opt.longrow_min_avg * n_rows && regular_cols < 0; }
  bool small_ok() const { return !wide; }
  bool small_pick(bool ok) const { return ok && (!has_rc || n_rows <= opt.small_over_rc); }
  bool sm_use() const { return small_pick(sm_ok); }
  bool smr_use() const { return smr_ok; }   // (transfers: measured ahead of the gather / staged-window forms up to small_max_rows - profiles/r05_small_levels.md)
  bool smp_use() const { return smp_ok; }
  // the same pass for a grid operator WITHOUT row classes (coefficients differ from row to row): structure classes + the
  // values in 7 planar arrays (build_band)
  bool rm3_var = false;
  DevBuf<double> vband;
  DevBuf<unsigned short> vb_cls;   // structure class of every row
  DevBuf<int> vb_slot;             // [class][entry] -> planar slot
  long long vstride = 0;
  long long band_ncls = 0;
  bool band_canon = false;         // slots in canonical order (-z, -y, -x, diagonal, +x, +y, +z): every class a 7-point star
  bool band_sym = false;           // ... and the values symmetric: the kernel reads the lower entries from the upper ones (March3Dev::vsrc)
  DevBuf<int> vb_bad;              // (scratch of the symmetry check)
  int rt_P = 0, rt_nplanes = 0, rt_halo = 0, rt_chunks = 0, rt_nblocks = 0;
  bool rt_lane = false;     // plane tiles with the per-lane walk of a padded LDS dictionary
  int rt_cr = mgk::RT_CR;   // rows of a plane per workgroup: 1024, or 256 on levels too small to fill the chip with 1024-row tiles
  // csr_rowclass_winp_spmv (prolongation-shaped operators: the source windows of a workgroup's rows staged in LDS)
  bool rp_ok = false;
  DevBuf<unsigned short> rp_wf;
  DevBuf<int> rp_cz0, rp_wlo, rp_code;
  int rp_PF = 0, rp_nplanes = 0, rp_PC = 0, rp_W = 0, rp_chunks = 0;
  mgk::WinPDev winpdev() const {
    mgk::WinPDev t;
    t.wf = rp_wf.p;
    t.cz0 = rp_cz0.p;
    t.wlo = rp_wlo.p;
    t.code = rp_code.p;
    t.PF = rp_PF;
    t.nplanes = rp_nplanes;
    t.PC = rp_PC;
    t.W = rp_W;
    t.chunks = rp_chunks;
    t.nblocks = rp_chunks * rp_nplanes;
    t.n_cols = (int)n_cols;
    t.ncls = (int)rc_ncls;
    t.nent = (int)rc_entries;
    t.maxlen = rc_maxlen;
    return t;
  }
  size_t winp_lds_bytes() const { return (size_t)2 * rp_W * 8 + (size_t)rc_ncls * (size_t)rc_maxlen * 16; }
  int rw_doubles = 0;   // x entries a workgroup of csr_rowclass_window_spmv stages in LDS
  DevBuf<unsigned short> rc_cls;
  DevBuf<double> rc_val, rc_d;
  bool has_rc = false;
  bool rc_implicit = false;   // first column = row + rc_delta[class]: no per-row first-column stream
  bool rc_has_d = false;      // the level's relaxPrec is constant per class: SMOOTH reads it from rc_d
  bool rc_window = false;     // csr_rowclass_window_spmv: the most frequent class's windows fit in LDS
  std::vector<unsigned short> h_cls;  // host class ids (to test vectors for class-constancy)
  long long rc_ncls = 0, rc_entries = 0;
  std::vector<int> h_rp, h_ci;  // host pattern, kept only while has_rc (to re-derive the classes for new values)
  std::vector<int> h_blk_row;  // host copy of the row-block boundaries (for building schedules)
  int max_row_nnz = 0;
  bool rows_sorted = true;   // every row's stored columns ascend (upload_csr): what rap_numeric needs of a coarse operator's pattern
  bool has_sched = false;
  int nblocks = 0;
  bool nt = false;  // non-temporal loads of the matrix stream (mg_kernels.hpp load_stream)
  // WIDE operator (round 6): >= 2^31 - 4096 non-zeros (or the option force_rowptr64: tests) - 64-bit row pointers, served by the two streaming
  // kernels (csr_stream_spmv / csr_longrow_spmv instantiated on CsrDev64), one right-hand side, no other format, no RAP / transpose on device
  DevBuf<long long> rowptr64;
  bool wide = false;
  mgk::CsrDev64 dev64() const {
    mgk::CsrDev64 d;
    d.rowptr = rowptr64.p;
    d.colidx = colidx.p;
    d.val = val.p;
    d.blk_row = blk_row.p;
    d.sched = nullptr;
    d.nblocks = nblocks;
    d.n_rows = (int)n_rows;
    d.n_cols = (int)n_cols;
    return d;
  }
  mgk::CsrDev dev() const {
    mgk::CsrDev d;
    d.rowptr = rowptr.p;
    d.colidx = colidx.p;
    d.val = val.p;
    d.blk_row = blk_row.p;
    d.sched = has_sched ? sched.p : nullptr;
    d.nblocks = nblocks;
    d.n_rows = (int)n_rows;
    d.n_cols = (int)n_cols;
    return d;
  }
  mgk::CsrDev dev_mm() const {
    mgk::CsrDev d = dev();
    d.blk_row = blk_row_mm.p;
    d.sched = has_sched_mm ? sched_mm.p : nullptr;
    d.nblocks = nblocks_mm;
    return d;
  }
  const double* d_bound = nullptr;   // the relaxPrec vector rc_d was derived from (mg_op_bind_relax_dev_FP64 / mg_finalize)
  bool rc_pair = false;     // plain row-class kernel with two consecutive rows per lane (alternating classes)
  // csr_rowclass_lane_spmv (every lane walks its own class, dictionary in LDS) replaces the waterfall kernel when the
  // dictionary fits
  bool rc_lane() const { return has_rc && !opt.no_lane && rc_ncls <= mgk::RL_NCLS && rc_entries <= mgk::RL_DCAP; }
  // block right-hand sides: csr_rowclass_lane_spmm when every row is in a dictionary class
  bool rc_lane_mm() const { return rc_lane() && !opt.no_lane_mm && rc_nexc == 0; }
  DevBuf<int> t_ptr, t_perm;   // transposed pattern (column -> entries in ascending row order): SPAI relaxPrec on the device
  bool has_t = false;
  DevBuf<int> sched_ln;     // L2-tiled order of the lane SpMM's row blocks (built for the current nrhs)
  bool has_sched_ln = false;
  int ln_rows = 0, ln_blocks = 0;
  int rc_blocks() const {
    const long long rows = rc_lane() ? mgk::RL_ROWS : (rc_pair ? 2 * mgk::BLK : mgk::RC_ROWS);
    return (int)((n_rows + rows - 1) / rows);
  }
  // workgroups of the nrhs == 1 product (one fused ||r||^2 partial each)
  int rw_blocks() const { return (int)((n_rows + mgk::RW_ROWS - 1) / mgk::RW_ROWS); }
  int exc_blocks() const { return rc_nexc > mgk::BLK ? (rc_nexc + mgk::BLK - 1) / mgk::BLK : 0; }   // short lists: in-kernel
  int blocks1() const { return has_rc ? (rc_march ? rm_nblocks : rc_tile ? rt_nblocks : rc_window ? rw_blocks() : rc_blocks()) + exc_blocks() : nblocks; }
  mgk::MarchDev marchdev() const {
    mgk::MarchDev t;
    t.lb = rm_lb.p;
    t.P = rm_P;
    t.nplanes = rm_nplanes;
    t.halo = rm_halo;
    t.chunks = rm_chunks;
    t.nblocks = rm_nblocks;
    t.n_cols = (int)n_cols;
    t.ncls = (int)rc_ncls;
    t.nent = (int)rc_entries;
    t.maxlen = rc_maxlen;
    return t;
  }
  int rc_maxlen = 0;        // longest class of the dictionary
  // Local operator of a sharded level: columns >= regular_cols are halo columns (appended after the owned ones); rows
  // that reference one are forced to be exception rows, the first regular_cols rows are the owned box in natural order
  long long regular_cols = -1;
  // rows >= regular_rows are empty halo rows (-1: the square box form, regular_rows == regular_cols; a prolongation over
  // [owned coarse | halo] columns has all its rows regular)
  long long regular_rows = -1;
  long long reg_rows() const { return regular_cols < 0 ? n_rows : (regular_rows >= 0 ? regular_rows : std::min(regular_cols, n_rows)); }
  mgk::TileDev tiledev() const {
    mgk::TileDev t;
    t.tile_lb = rt_lb.p;
    t.P = rt_P;
    t.nplanes = rt_nplanes;
    t.halo = rt_halo;
    t.chunks = rt_chunks;
    t.nblocks = rt_nblocks;
    t.n_cols = (int)n_cols;
    t.lane = rt_lane ? 1 : 0;
    t.ncls = (int)rc_ncls;
    t.maxlen = rc_maxlen;
    return t;
  }
  size_t tile_lds_bytes() const {
    return (size_t)(mgk::RT_NP + 2) * (size_t)(rt_cr + 2 * rt_halo) * sizeof(double) +
           (rt_lane ? (size_t)rc_ncls * (size_t)rc_maxlen * 16 + (size_t)rc_ncls * 8 : 0);
  }
  mgk::RowClassDev rcdev() const {
    mgk::RowClassDev c;
    c.firstcol = rc_implicit ? nullptr : rc_first.p;
    c.cls_delta = rc_delta.p;
    c.cls_d = rc_d.p;
    c.exc_rows = rc_exc.p;
    c.nexc_inline = (rc_nexc > 0 && rc_nexc <= mgk::BLK) ? rc_nexc : 0;
    c.rowptr = rowptr.p;
    c.colidx = colidx.p;
    c.val = val.p;
    c.cls = rc_cls.p;
    c.cls_ptr = rc_ptr.p;
    c.cls_off = rc_off.p;
    c.cls_val = rc_val.p;
    c.nblocks = rc_blocks();
    // a box operator's rows beyond the owned box are empty halo rows: no kernel may touch them - the row operands (b, d, y)
    // are only n_own long, and "a safe row" for idle lanes must be one of the owned rows
    c.n_rows = (int)reg_rows();
    return c;
  }
  void drop_rc() {
    rc_first.release();
    rc_ptr.release();
    rc_off.release();
    rc_cls.release();
    rc_val.release();
    rc_delta.release();
    rw_meta.release();
    rw_lb.release();
    rt_lb.release();
    rm_lb.release();
    rc_exc.release();
    rc_nexc = 0;
    rc_tile = false;
    rc_march = false;
    rc_march2 = false;
    rc_march3 = false;
    rm3_var = false;
    vband.release();
    vb_cls.release();
    vb_slot.release();
    vb_bad.release();
    band_canon = band_sym = false;
    rm3_cls.release();
    rm3_cmap.release();
    rc_march4 = false;
    rm4_cls.release();
    rm4_ysh.release();
    rc_marchr = false;
    rmr_cls.release();
    rmr_cmap.release();
    rc_march27 = false;
    rm27_cls.release();
    rm27_cmap.release();
    rm27_sink.release();
    rc_exc2.release();
    rc_nexc2 = 0;
    rp_ok = false;
    rp_wf.release();
    h_rc_ptr.clear();
    h_rc_off.clear();
    h_rc_delta.clear();
    rc_d.release();
    h_cls.clear();
    h_cls.shrink_to_fit();
    has_rc = false;
    rc_implicit = false;
    rc_has_d = false;
    rc_window = false;
    rc_pair = false;
    rc_ncls = rc_entries = 0;
  }
  mgk::PatDev patdev() const {
    mgk::PatDev p;
    p.firstcol = firstcol.p;
    p.pat = pat.p;
    p.pat_ptr = pat_ptr.p;
    p.pat_off = pat_off.p;
    p.dict_entries = (int)dict_entries;
    p.npat = (int)npat;
    p.run_ptr = has_runs ? run_ptr.p : nullptr;
    p.runs = has_runs ? runs.p : nullptr;
    return p;
  }
  void release() {
    drop_rc();
    sm_ok = smr_ok = smp_ok = false;
    cellp_ok = false;
    waver_ok = false;
    b27_ok = false;
    b27_val.release();
    b27_flag.release();
    ci16.release();
    rowbase.release();
    rowptr64.release();
    wide = false;
    has_ci16 = false;
    sm_rec.release();
    smr_rec.release();
    sm_d_bound = nullptr;
    h_rp.clear();
    h_rp.shrink_to_fit();
    h_ci.clear();
    h_ci.shrink_to_fit();
    run_ptr.release();
    runs.release();
    has_runs = false;
    firstcol.release();
    pat_ptr.release();
    pat_off.release();
    pat.release();
    has_pat = false;
    t_ptr.release();
    t_perm.release();
    has_t = false;
    rowptr.release();
    colidx.release();
    blk_row.release();
    sched.release();
    has_sched = false;
    blk_row_mm.release();
    sched_mm.release();
    has_sched_mm = false;
    val.release();
    set = false;
  }
  size_t bytes() const {
    return blk_row_mm.bytes() + sched_mm.bytes() + rowptr.bytes() + colidx.bytes() + blk_row.bytes() + val.bytes() + sched.bytes() + firstcol.bytes() +
           pat_ptr.bytes() + pat_off.bytes() + pat.bytes() + run_ptr.bytes() + runs.bytes();
  }
};

struct VankaCore;   // mg_vanka.inc: geometry, blocks and delta buffer of the Vanka smoother

struct Level {
  VankaCore* vanka = nullptr;   // relaxation type 2: bound by mg_set_vanka_FP64, released by mg_destroy
  int vanka_type = 0;
  long long grid[3] = {0, 0, 0};  // optional hint: the rows are an x-fastest n1 x n2 x n3 nodal grid
  Csr A, P, R;  // P, R: transfer to/from the next coarser level (unset on the coarsest)
  DevBuf<double> d;
  bool relax_set = false;
  long long npre = 1, npost = 1;
  long long n = 0;
  // (the vectors a cycle plays in - b, r, x0, x1 - are per lane: Play)
  DevBuf<double> x2;   // fine level, solve loop: third rotating buffer of the fused last sweep + residual (allocated on first use)
  DevBuf<double> x3;   // scratch for outputs of the fused sweep + residual nobody asked for (test entry point only)
  // FGMRESmem (FGMRES.jl:3-8): Z and A*Z bases, `inner` contiguous vectors of n*nrhs each.
  // relaxZ/relaxAZ: memRelax[level] (Jac-GMRES smoother); kZ/kAZ: memKcycle (K-cycle recursion INTO this level)
  DevBuf<double> relaxZ, relaxAZ, kZ, kAZ;
  long long relax_inner = 0;
};

// What a cycle plays in: a stream, the reduction buffers and the vectors of every level.  The handle's own lane (lane 0) is as wide
// as the handle; the further lanes of the column-wise block solve (solve_dev_columns) hold one column each, so that one column's
// launch-bound coarse levels and kernel ramps run under another's fine-level kernels.
struct Play {
  hipStream_t stream = nullptr;
  bool owns_stream = true;         // the library created it (mg_set_stream: the caller's)
  DevBuf<double> partial, partial2, scalar;   // reductions
  bool scalar_mirrored = false;    // the kernel that produced `scalar` also stored it into the handle's pinned h_scalar (sum_final_mirror)
  // CYCLEmem (MGdef.jl:56-60) plus the Jacobi ping-pong partner of x
  struct Vecs { DevBuf<double> b, r, x0, x1; };
  std::vector<Vecs> lev;
  // not owned
  long long nrhs = 1;              // columns per vector the kernels see: 1 while a block is played column by column, else the handle's
  double* r0 = nullptr;            // fine-level residual in use: the lane's own, or a column's slice of colbuf[3]
  double* res(int l) const { return l == 0 ? r0 : lev[(size_t)l].r.p; }
  void rest(long long width) {     // (no column in play)
    nrhs = width;
    r0 = lev.empty() ? nullptr : lev[0].r.p;
  }
  int alloc(const mg_hierarchy* h, long long width, bool fine);
  void release_vectors() {
    for (Vecs& V : lev)
      for (DevBuf<double>* d : {&V.b, &V.r, &V.x0, &V.x1}) d->release();
    r0 = nullptr;
  }
  void release() {
    release_vectors();
    for (DevBuf<double>* d : {&partial, &partial2, &scalar}) d->release();
    if (stream && owns_stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
  }
};

struct ProfSlot {
  double ms = 0.0;
  long long launches = 0;
  double bytes = 0.0;   // algorithmic (CSR-priced) bytes, SURVEY 8d: SUM over the launches (reported per launch = / launches)
  double moved = 0.0;   // bytes the kernel IN USE has to move (device format + each vector once): SUM over the launches
};

}  // namespace

struct mg_ghost;   // (mg_ghost.inc) geometry, plans and transport of the ghost-layer form of the sharded cycle
struct CxState;   // mg_complex.inc: the levels of a ComplexF64 handle
struct mg_dd;     // mg_dd.inc: the multiplicative Schwarz sweep (a hierarchy may borrow one as its coarsest solve)

struct mg_hierarchy {
  Options opt;
  CxState* cx = nullptr;       // set by mg_create_CF64: the value type is ComplexF64 and the real levels stay empty
  mg_ghost* ghost = nullptr;   // set by mg_ghost_attach: this hierarchy is one rank's part (extended boxes) of a sharded one
  int device = 0;
  long long nlevels = 0;
  long long nrhs = 1;
  char cycle = 'V';
  int relax_type = 0;  // 0: pointwise d (Jac / SPAI, MGcycle.jl:122-136); 1: Jac-GMRES (FGMRES.jl:48-126); 2: Vanka (Vanka.jl:372-434)
  bool finalized = false;
  std::vector<Level> lev;
  DevBuf<double> Ainv;  // row-major n_c x n_c
  long long n_coarse = 0;
  bool coarse_set = false;
  // sparse-factor form of the coarsest solve (parLU layout), used instead of Ainv when coarse_lu is true
  bool coarse_lu = false;
  DevBuf<int> luLptr, luLcol, luUptr, luUcol, luP, luQ, luLorder, luLlvl, luUorder, luUlvl;
  DevBuf<double> luLval, luUval, luWork;
  int nLlvl = 0, nUlvl = 0;
  // chip-wide form (factors of >= lu_multi_min_rows rows): host copies of the level pointers for the per-level
  // launches, and the explicit inverses of the dense trailing blocks (rows n-luML.. of L, n-luMU.. of U)
  std::vector<int> luLlvl_h, luUlvl_h;
  DevBuf<double> luInvL, luInvU, luTail;
  DevBuf<int> luLslot, luUslot;   // per level slot {row, first, end of the off-diagonal entries, diagonal entry}
  int luML = 0, luMU = 0;
  bool lu_multi = false;
  bool lu_only = false;     // a stand-alone factor applier (mg_lu_*): one "level" that consists of the coarsest solve only
  // launch-bound coarse sub-cycles replay as HIP graphs (captured on first use; keyed by level, buffers and cycle)
  struct GraphKey {
    int level; bool x_zero; char ctype; const void* b; const void* xa; const void* xb; bool x1_given;
    long long nrhs;
    bool operator<(const GraphKey& o) const {
      return std::tie(level, x_zero, ctype, b, xa, xb, x1_given, nrhs) < std::tie(o.level, o.x_zero, o.ctype, o.b, o.xa, o.xb, o.x1_given, o.nrhs);
    }
  };
  struct GraphEntry { hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; double* result = nullptr; };
  std::map<GraphKey, GraphEntry> graphs;
  bool capturing = false;
  long long graph_launches = 0;
  Play lane0;                  // the handle's own lane
  std::vector<Play*> lanes;    // solve_dev_columns: lanes 1..S-1 (column c plays in lane c mod S), without fine-level vectors
  std::vector<hipEvent_t> lane_ready;   // ... and the event behind which each of them starts (the transposes)
  Play* play = &lane0;         // not owned: the lane being played (set for a scope by Lane)
  DevBuf<double> m3sink;       // csr_rowclass_march3_spmv: one slot per lane for the stores of lanes with nothing to store
  DevBuf<double> colbuf[4];    // solve_dev_columns: b, x, the second iterate buffer and r as k columns of stride ns
  double* h_cols = nullptr;    // pinned: ||r_c||^2 of every column of the step in flight
  long long h_cols_n = 0;
  double* h_scalar = nullptr;  // pinned: [0] the scalar of scalar_sync / dot_sync; [1], [2] the norms of the pipelined solve loop
  hipEvent_t pipe_ev[2] = {nullptr, nullptr};   // ... and the events behind them
  struct DeferredSum { bool on = false; int np = 0; double* host = nullptr; hipEvent_t ev = nullptr; } dsum;   // the four-stage pass's final sum, left to the next launch (k_four_stage / k_spmv)
  int nred_blocks = 1024;
  // staging for the host-pointer API
  DevBuf<double> stage_b, stage_x, stage_t;
  // Krylov work vectors (allocated on the first mg_pcg call)
  DevBuf<double> kr, kz, kp, kAp, kw;
  DevBuf<double> blk_partial, blk_c;   // block Krylov: Gram partials, coefficient slots
  double* h_blk = nullptr;             // pinned k x k readback
  double* h_blk_c = nullptr;           // pinned ring of coefficient matrices
  unsigned blk_c_next = 0;
  DevBuf<double> kwc_blk;   // the same for a block of right-hand sides (blockFGMRES branch, MGcycle.jl:166)
  DevBuf<double> kscal;     // FGMRES: the Hessenberg column of an inner step, on the device
  double* h_kscal = nullptr;   // ... and its pinned readback (66 doubles)
  DevBuf<double> kstepZ, kstepAZ, kstepX;   // mg_kcycle_step_async_dev_FP64: the K-step INTO this hierarchy's first level
  DevBuf<double> kwc, coarse_d;   // coarseSolveType "GMRES": FGMRES work space and the Jacobi preconditioner of the coarsest level
  bool coarse_gmres = false;
  mg_dd* coarse_dd = nullptr;   // mg_set_coarse_dd: the coarsest solve is one Schwarz sweep of this (borrowed) handle; both value types
  // fine-level operands of the last cycle/solve (used as inputs by mg_time_op_dev_FP64)
  const double* last_b = nullptr;
  double* last_x = nullptr;
  // profiling
  bool prof = false;
  std::vector<ProfSlot> slots;  // [level][kernel]
  struct Pending {
    hipEvent_t a, b;
    int level, kernel;
    double bytes, moved;
  };
  std::vector<Pending> pending;
  std::vector<hipEvent_t> ev_pool;
};

namespace {
// The lane's level vectors for `width` columns (fine: the fine level's r and x1 too), its reduction buffers as large as lane 0's and,
// unless it plays on a caller's stream, a stream of its own.  A buffer whose size changes is allocated anew and zeroed.
int Play::alloc(const mg_hierarchy* h, long long width, bool fine) {
  if (!stream && owns_stream) HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  lev.resize((size_t)h->nlevels);
  for (int l = fine ? 0 : 1; l < (int)h->nlevels; ++l) {
    const size_t len = (size_t)h->lev[(size_t)l].n * (size_t)width;
    Vecs& V = lev[(size_t)l];
    for (DevBuf<double>* d : {&V.r, &V.x1, &V.b, &V.x0}) {
      if (l == 0 && (d == &V.b || d == &V.x0)) continue;   // (the fine b and x are the caller's)
      if (d->n == std::max<size_t>(1, len)) continue;
      MG_TRY(d->alloc(len));
      HIP_TRY(hipMemset(d->p, 0, d->bytes()));
    }
  }
  // (the fused residual + norm writes one partial per row block of the fine operator)
  const size_t np = std::max({h->lane0.partial.n, (size_t)h->nred_blocks, (size_t)h->lev[0].A.nblocks, (size_t)h->lev[0].A.ln_blocks});
  if (partial.n != np) MG_TRY(partial.alloc(np));
  if (partial2.n != 256) MG_TRY(partial2.alloc(256));
  if (scalar.n != 1) MG_TRY(scalar.alloc(1));
  rest(width);
  return MG_OK;
}

// Plays lane `si` for its lifetime, `width` columns per vector, the fine-level residual at r (nullptr: the lane's own).  Afterwards the
// handle plays its own lane again, at its own width.
struct Lane {
  mg_hierarchy* h;
  Lane(mg_hierarchy* h_, int si, long long width, double* r = nullptr) : h(h_) {
    h->play = si == 0 ? &h->lane0 : h->lanes[(size_t)si - 1];
    h->play->nrhs = width;
    if (r) h->play->r0 = r;
  }
  Lane(const Lane&) = delete;
  ~Lane() {
    h->play = &h->lane0;
    h->lane0.rest(h->nrhs);
  }
};
}  // namespace
