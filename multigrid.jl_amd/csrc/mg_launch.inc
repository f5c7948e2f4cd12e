// mg_launch.inc - part of libmgvcycle.so's single translation unit (included by mgvcycle.hip in this order; not compiled on its own).
// Byte accounting, HIP-event profiling slots, kernel launchers (format dispatch of every product / sweep / residual), norms.
namespace {

// ---------------------------------------------------------------------------------------------
// algorithmic bytes (DESIGN.md section 5): int32 indices + fp64 values, each vector element once
// ---------------------------------------------------------------------------------------------
double spmv_bytes(const Csr& M, long long nrhs, bool reads_y_or_b, bool smooth) {
  double bts = 12.0 * (double)M.nnz + 4.0 * (double)(M.n_rows + 1);
  bts += 8.0 * (double)nrhs * (double)(M.n_cols + M.n_rows);  // x read, y written
  if (reads_y_or_b) bts += 8.0 * (double)nrhs * (double)M.n_rows;
  if (smooth) bts += 8.0 * (double)M.n_rows;  // d; the x[row] term is the already-counted x read
  return bts;
}

// Matrix-side bytes one launch of the kernel IN USE streams for M (the device format chosen at upload).
double format_bytes(const Csr& M, long long nrhs) {
  if (nrhs == 1 && (M.cellp_ok || M.waver_ok)) return 0.0;   // arithmetic transfer kernels (grid_cell_prolong / grid_wave_restrict): no matrix side at all
  if (M.has_rc && nrhs == 1 && M.rp_ok)   // LDS-staged prolongation: class id + 16-bit window index per row
    return 4.0 * (double)M.n_rows + 12.0 * (double)M.rc_entries;
  if (M.has_rc && nrhs == 1 && M.rc_march27 && !M.opt.no_march27)       // 27-point marching form: class records + index maps, no per-row stream
    return 224.0 * (double)M.rc_ncls + 2.0 * (double)(M.rm27[0].n1 + M.rm27[0].n2 + M.rm27[0].nplanes + M.rm27[0].ntab);
  if (M.has_rc && (nrhs == 1 || (M.rc_lane_mm() && M.ln_blocks > 0)))   // (block right-hand sides: the lane SpMM)
    return (M.rc_implicit ? 2.0 : 6.0) * (double)M.n_rows + 12.0 * (double)M.rc_entries;
  if (nrhs == 1 && M.b27_ok && !M.has_rc)   // band-27: planar value arrays, 14 of the 27 where the symmetric reads serve the operator
    return 8.0 * (double)(M.b27.sym ? 14 : 27) * (double)M.n_rows;
  if (nrhs == 1 && M.has_pat)
    return 8.0 * (double)M.nnz + 4.0 * (double)M.dict_entries +
           (M.has_runs ? 20.0 * (double)M.nruns_total + 8.0 * (double)M.nblocks : 10.0 * (double)M.n_rows);
  return 12.0 * (double)M.nnz + 4.0 * (double)(M.n_rows + 1);
}
// Compulsory bytes of one launch in that format: the matrix side above + every vector element once
// (class_d: the relaxPrec comes from the class dictionary instead of an 8 B/row stream).
double moved_bytes(const Csr& M, long long nrhs, bool reads_y_or_b, bool smooth, bool class_d = false) {
  double bts = format_bytes(M, nrhs) + 8.0 * (double)nrhs * (double)(M.n_cols + M.n_rows);
  if (reads_y_or_b) bts += 8.0 * (double)nrhs * (double)M.n_rows;
  if (smooth && !class_d) bts += 8.0 * (double)M.n_rows;
  return bts;
}

int grid_for(long long total) {
  long long g = (total + mgk::BLK - 1) / mgk::BLK;
  return (int)std::max<long long>(1, std::min<long long>(g, 2048));
}

// ghost-layer form of the sharded cycle (mg_ghost.inc, defined behind this part)
void gh_own_box(const mg_hierarchy* h, int level, int* xl, int* xh, int* yl, int* yh, int* zl, int* zh);
bool gh_global_scalars(const mg_hierarchy* h);
int gh_scalar_to_slot(mg_hierarchy* h, double* slot);

// ---- profiling helpers --------------------------------------------------------------------------
hipEvent_t get_event(mg_hierarchy* h) {
  if (!h->ev_pool.empty()) {
    hipEvent_t e = h->ev_pool.back();
    h->ev_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

// h->play->scalar = sum of np partials, also stored straight into the pinned h_scalar (scalar_sync then needs no copy)
void launch_sum_final(mg_hierarchy* h, const double* partial, int np) {
  hipLaunchKernelGGL(mgk::sum_final_mirror, dim3(1), dim3(mgk::BLK), 0, h->play->stream, partial, np, h->play->scalar.p, h->h_scalar);
  h->play->scalar_mirrored = !h->capturing;
}
struct ProfScope {
  mg_hierarchy* h;
  bool on;
  mg_hierarchy::Pending p;
  ProfScope(mg_hierarchy* h_, int level, int kernel, double bytes, double moved = -1.0) : h(h_), on(h_->prof) {
    if (!on) return;
    p.a = get_event(h);
    p.b = get_event(h);
    p.level = level;
    p.kernel = kernel;
    p.bytes = bytes;
    p.moved = moved < 0.0 ? bytes : moved;
    (void)hipEventRecord(p.a, h->play->stream);
  }
  ~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(p.b, h->play->stream);
    h->pending.push_back(p);
  }
};

void prof_collect(mg_hierarchy* h) {
  for (auto& p : h->pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      ProfSlot& s = h->slots[(size_t)p.level * MG_K_COUNT + p.kernel];
      s.ms += ms;
      s.launches += 1;
      s.bytes += p.bytes;   // (launches of one slot may differ: the fused sweep + residual writes r, x + d.*r or neither)
      s.moved += p.moved;
    }
    h->ev_pool.push_back(p.a);
    h->ev_pool.push_back(p.b);
  }
  h->pending.clear();
}

// ---- kernel launchers ---------------------------------------------------------------------------
int pow2_ge(long long v) {
  int g = 1;
  while (g < v && g < 64) g <<= 1;
  return g;
}

// csr_rowclass_march3_spmv: 16-byte pairs of a slab per lane
constexpr int RM3_NPM = 2;
// dynamic LDS of csr_rowclass_march2_spmv: 4 x slabs + 4 t slabs + dictionary
size_t march2_lds_bytes(int halo) {
  const size_t slx = (size_t)(mgk::RM_C + 4 * halo + 2), slt = (size_t)(mgk::RM_C + 2 * halo);
  return (4 * slx + 4 * slt) * sizeof(double) + 16 * (size_t)mgk::RM_DCAP + 8 * (size_t)mgk::RM_NCLS + 4 * (size_t)(mgk::RM_NCLS + 4);
}

// can the z-marching kernel serve this launch?  (staged variants read x workgroup-wide: never in place; its staging
// loads are 16 bytes wide: x must be 16-byte aligned, which every allocation base is)
// 27-point marching form (csr_rowclass_march27_spmv): TWO = sweep + residual, else one product (MODE1 = SMOOTH / RESID)
static int big_lds_attr(const void* fn, std::atomic<unsigned long long>& done, size_t bytes = 160 * 1024 - 256);
template <bool TWO, int MODE1, int NT, int PITCH, bool FZ>
int launch_march27_p(hipStream_t stream, const Csr& A, const mgk::March2Args& a) {
  auto* fn = &mgk::csr_rowclass_march27_spmv<TWO, MODE1, NT, 1, PITCH, FZ>;
  static std::atomic<unsigned long long> attr_done{0};
  MG_TRY(big_lds_attr(reinterpret_cast<const void*>(fn), attr_done, 160 * 1024 - 256));
  const int g = TWO ? 1 : 0;
  hipLaunchKernelGGL(fn, dim3((unsigned)A.rm27[g].nblocks), dim3(NT), A.rm27_lds[g], stream, a, A.rm27[g]);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
template <bool TWO, int MODE1, int NT, bool FZ>
int launch_march27_n(hipStream_t stream, const Csr& A, const mgk::March2Args& a) {
  switch (A.rm27_pitch[TWO ? 1 : 0]) {
    case 24: return launch_march27_p<TWO, MODE1, NT, 24, FZ>(stream, A, a);
    case 32: return launch_march27_p<TWO, MODE1, NT, 32, FZ>(stream, A, a);
    case 40: return launch_march27_p<TWO, MODE1, NT, 40, FZ>(stream, A, a);
    case 48: return launch_march27_p<TWO, MODE1, NT, 48, FZ>(stream, A, a);
    case 64: return launch_march27_p<TWO, MODE1, NT, 64, FZ>(stream, A, a);
  }
  return fail(MG_ERR_STATE, "27-point marching form: slab pitch %d is not instantiated", A.rm27_pitch[TWO ? 1 : 0]);
}
template <bool TWO, int MODE1, bool FZ = false>
int launch_march27(hipStream_t stream, const Csr& A, mgk::March2Args a) {
  a.sink = A.rm27_sink.p;
  const int g = TWO ? 1 : 0;
  if (A.rm27_nt[g] == 1024) return launch_march27_n<TWO, MODE1, 1024, FZ>(stream, A, a);
  if (A.rm27_nt[g] == 512) return launch_march27_n<TWO, MODE1, 512, FZ>(stream, A, a);
  if (A.rm27_nt[g] == 256) return launch_march27_n<TWO, MODE1, 256, FZ>(stream, A, a);
  return fail(MG_ERR_STATE, "27-point marching form: %d threads is not instantiated", A.rm27_nt[g]);
}
// marching restriction (csr_rowclass_marchr_spmv): y = R x [, y2 = d2 .* y] for alpha = 1, beta = 0, one right-hand side
bool marchr_ok(const Csr& M, const mgk::VecArgs& v) {
  return v.nrhs == 1 && M.has_rc && M.rc_marchr && !M.opt.no_marchr && v.alpha == 1.0 && v.beta == 0.0 && v.y && v.y != v.x && !v.sumsq &&
         (!v.y2 || v.d_full) && (reinterpret_cast<uintptr_t>(v.x) & 15) == 0;
}
int launch_marchr(hipStream_t stream, const Csr& M, const mgk::VecArgs& v) {
  mgk::March2Args a{};
  a.x = v.x;
  a.t = v.y;
  a.xn = v.y2;
  a.d = v.y2 ? v.d_full : nullptr;
  a.sink = M.rm27_sink.p;
  auto* fn = &mgk::csr_rowclass_marchr_spmv<256, 3, 72>;
  hipLaunchKernelGGL(fn, dim3((unsigned)M.rmr.nblocks), dim3(256), M.rmr_lds, stream, a, M.rmr);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
// one product on the 27-point form: a single vector, class relaxPrec, out of place, x 16-byte aligned, no ||.||^2, no second output
template <int MODE>
bool march27_single_ok(const Csr& M, const mgk::VecArgs& v) {
  return (MODE == mgk::SMOOTH || MODE == mgk::RESID) && v.nrhs == 1 && M.has_rc && M.rc_march27 && !M.opt.no_march27 && M.rc_nexc == 0 && v.y && v.y != v.x &&
         !v.y2 && !v.sumsq && (v.xs == nullptr || v.xs == v.x) && (MODE != mgk::SMOOTH || !v.d) && (reinterpret_cast<uintptr_t>(v.x) & 15) == 0;
}
bool march_ok(const Csr& M, const mgk::VecArgs& v) {
  return v.nrhs == 1 && M.has_rc && M.rc_march && v.y != v.x && v.y2 != v.x && (v.xs == nullptr || v.xs == v.x) &&
         (reinterpret_cast<uintptr_t>(v.x) & 15) == 0;
}

// nparts (optional): number of per-workgroup ||out||^2 partials the launch writes to v.sumsq.
// phase: 0 = the whole product; 1 = every row that is in a dictionary class; 2 = the exception rows only (the sharded
// cycle computes the rows that read the halo - forced exception rows - after the exchange has landed).  Operators that
// are not stored as row classes compute everything in phase 2.
// Lane SpMM: lanes per row.  Even nrhs: two columns (16 bytes) per lane, G = pow2 >= nrhs/2 lanes per row.
static inline bool lane_mm_pairs(const Csr& M, long long nrhs) { return nrhs % 2 == 0 && !M.opt.no_lane_pairs; }
static inline int lane_mm_group(const Csr& M, long long nrhs) { return lane_mm_pairs(M, nrhs) ? pow2_ge(nrhs / 2) : pow2_ge(nrhs); }
// rows per lane of the row-class SpMM: 3 for a square operator in the paired-column form (A: sweeps, residuals), else 2
static inline int lane_mm_rpl(const Csr& M, long long nrhs) { return (lane_mm_pairs(M, nrhs) && M.n_rows == M.n_cols && !M.opt.no_lane_rpl3) ? 3 : 2; }
static inline bool aligned16(const mgk::VecArgs& v) {
  auto ok = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
  return ok(v.x) && ok(v.y) && ok(v.b) && ok(v.xs);
}
template <int MODE>
int launch_csr(hipStream_t stream, const Csr& M, const mgk::VecArgs& v, int* nparts = nullptr, int phase = 0) {
  if (nparts) *nparts = M.nblocks;
  if (M.nblocks <= 0) return MG_OK;
  if (M.wide) {   // >= 2^31 non-zeros: 64-bit row pointers, the two streaming kernels
    if (v.nrhs != 1) return fail(MG_ERR_UNSUPPORTED, "an operator with 64-bit row pointers (>= 2^31 non-zeros) serves one right-hand side at a time");
    if (phase == 1) {
      if (nparts) *nparts = 0;
      return MG_OK;
    }
    if (!v.sumsq && v.y && v.y != v.x && M.longrow() && (MODE != mgk::AXPBY || !v.y2 || v.d_full) && (MODE != mgk::SMOOTH || (v.d_full && v.xs))) {
      int dev = 0, ncu = 256;
      (void)hipGetDevice(&dev);
      (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
      const long long want = (long long)ncu * 8 * 4;
      const int rpw = (int)std::max<long long>(4, ((M.n_rows + want - 1) / want + 3) / 4 * 4);
      const int nwg = (int)((M.n_rows + rpw - 1) / rpw);
      if (M.nt) hipLaunchKernelGGL((mgk::csr_longrow_spmv<MODE, true, false, mgk::CsrDev64>), dim3(nwg), dim3(mgk::BLK), 0, stream, M.dev64(), v, nwg, rpw, nullptr, nullptr);
      else hipLaunchKernelGGL((mgk::csr_longrow_spmv<MODE, false, false, mgk::CsrDev64>), dim3(nwg), dim3(mgk::BLK), 0, stream, M.dev64(), v, nwg, rpw, nullptr, nullptr);
      if (nparts) *nparts = 0;
    } else {
      mgk::VecArgs w = v;
      if (MODE == mgk::SMOOTH && !w.d) w.d = w.d_full;
      if (M.nt) hipLaunchKernelGGL((mgk::csr_stream_spmv<MODE, true, mgk::CsrDev64>), dim3(M.nblocks), dim3(mgk::BLK), 0, stream, M.dev64(), w);
      else hipLaunchKernelGGL((mgk::csr_stream_spmv<MODE, false, mgk::CsrDev64>), dim3(M.nblocks), dim3(mgk::BLK), 0, stream, M.dev64(), w);
    }
    HIP_TRY(hipGetLastError());
    return MG_OK;
  }
  if (v.nrhs == 1 && phase == 0 && !v.sumsq && v.y && v.y != v.x) {   // small grid levels: one trip to memory per launch (mg_small.hpp)
    auto small_grid = [](long long rows, unsigned* nt) {
      *nt = rows <= 40000 ? 64u : 256u;      // (tiny levels: one wavefront per workgroup, spread over the CUs)
      return dim3((unsigned)((rows + *nt - 1) / *nt));
    };
    unsigned nt = 256;
    if (MODE != mgk::AXPBY && M.sm_use() && !v.y2 && (v.xs == nullptr || v.xs == v.x) && (MODE != mgk::SMOOTH || (!v.d && M.sm_d_bound))) {
      const dim3 g = small_grid(M.n_rows, &nt);
      hipLaunchKernelGGL((mgk::grid27_small_spmv<MODE>), g, dim3(nt), 0, stream, M.sm, v.x, v.b, v.y);
      if (nparts) *nparts = 0;
      HIP_TRY(hipGetLastError());
      return MG_OK;
    }
    if (M.b27_ok && !v.y2 && (MODE != mgk::SMOOTH || (v.d_full && v.xs))) {   // variable-coefficient 27-point grid operator: planar values
      hipLaunchKernelGGL((mgk::grid27_band_spmv<MODE>), dim3((unsigned)(((M.n_rows + 61) / 62 + 3) / 4)), dim3(256), 0, stream, M.b27, v);   // 62 rows per wavefront
      if (nparts) *nparts = 0;
      HIP_TRY(hipGetLastError());
      return MG_OK;
    }
    if (MODE == mgk::AXPBY && M.sm_use() && v.alpha == 1.0 && v.beta == 0.0 && !v.y2) {
      const dim3 g = small_grid(M.n_rows, &nt);
      hipLaunchKernelGGL((mgk::grid27_small_spmv<mgk::AXPBY>), g, dim3(nt), 0, stream, M.sm, v.x, nullptr, v.y);
      if (nparts) *nparts = 0;
      HIP_TRY(hipGetLastError());
      return MG_OK;
    }
    // (16-byte pairs of the fine vector: an aligned base - the pair at its last, odd-length entry then stays inside one 16-byte granule)
    if (MODE == mgk::AXPBY && M.waver_ok && v.alpha == 1.0 && v.beta == 0.0 && (!v.y2 || v.d_full) && (reinterpret_cast<uintptr_t>(v.x) & 15) == 0) {   // 62 coarse nodes per wavefront
      const long long waves = (M.n_rows + 61) / 62;
      hipLaunchKernelGGL(mgk::grid_wave_restrict, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, M.smr, M.waver_scale, v.x, v.y,
                         v.y2 ? v.d_full : nullptr, v.y2, mgk::FinalSum{nullptr, 0, nullptr, nullptr});
      if (nparts) *nparts = 0;
      HIP_TRY(hipGetLastError());
      return MG_OK;
    }
    if (MODE == mgk::AXPBY && M.smr_use() && v.alpha == 1.0 && v.beta == 0.0 && (!v.y2 || v.d_full)) {
      const dim3 g = small_grid(M.n_rows, &nt);
      hipLaunchKernelGGL(mgk::grid27_small_restrict, g, dim3(nt), 0, stream, M.smr, v.x, v.y, v.y2 ? v.d_full : nullptr, v.y2);
      if (nparts) *nparts = 0;
      HIP_TRY(hipGetLastError());
      return MG_OK;
    }
    if (MODE == mgk::AXPBY && M.cellp_ok && v.alpha == 1.0 && v.beta == 1.0 && !v.y2 && v.y != v.x && (reinterpret_cast<uintptr_t>(v.y) & 15) == 0) {   // a lane per coarse cell (16-byte pairs of x)
      hipLaunchKernelGGL(mgk::grid_cell_prolong, dim3((unsigned)(((long long)M.smp.m1 * M.smp.m2 * M.smp.m3 + 255) / 256)), dim3(256), 0, stream, M.smp, v.x, v.y);
      if (nparts) *nparts = 0;
      HIP_TRY(hipGetLastError());
      return MG_OK;
    }
    if (MODE == mgk::AXPBY && M.smp_use() && v.alpha == 1.0 && v.beta == 1.0 && !v.y2) {
      const dim3 g = small_grid(M.n_rows, &nt);
      hipLaunchKernelGGL(mgk::grid_small_prolong, g, dim3(nt), 0, stream, M.smp, v.x, v.y);
      if (nparts) *nparts = 0;
      HIP_TRY(hipGetLastError());
      return MG_OK;
    }
  }
  const dim3 grid(M.nblocks), blk(mgk::BLK);
  if (v.nrhs == 1 && phase == 0 && !v.sumsq && v.y && v.y != v.x && M.longrow() && (MODE != mgk::AXPBY || !v.y2 || v.d_full) &&
      (MODE != mgk::SMOOTH || (v.d_full && v.xs))) {
    // long rows (SA-AMG middle levels): one wavefront per row, bands of rows per workgroup - about four bands per CU slot
    int dev = 0, ncu = 256;
    (void)hipGetDevice(&dev);
    static int ncu_cached[64] = {0};
    if (!ncu_cached[dev & 63]) { (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev); ncu_cached[dev & 63] = ncu; }
    ncu = ncu_cached[dev & 63];
    const long long want = (long long)ncu * 8 * 4;
    const int rpw = (int)std::max<long long>(4, ((M.n_rows + want - 1) / want + 3) / 4 * 4);
    const int nwg = (int)((M.n_rows + rpw - 1) / rpw);
    if (M.has_ci16) {
      if (M.nt) hipLaunchKernelGGL((mgk::csr_longrow_spmv<MODE, true, true>), dim3(nwg), blk, 0, stream, M.dev(), v, nwg, rpw, M.ci16.p, M.rowbase.p);
      else hipLaunchKernelGGL((mgk::csr_longrow_spmv<MODE, false, true>), dim3(nwg), blk, 0, stream, M.dev(), v, nwg, rpw, M.ci16.p, M.rowbase.p);
    } else {
      if (M.nt) hipLaunchKernelGGL((mgk::csr_longrow_spmv<MODE, true, false>), dim3(nwg), blk, 0, stream, M.dev(), v, nwg, rpw, nullptr, nullptr);
      else hipLaunchKernelGGL((mgk::csr_longrow_spmv<MODE, false, false>), dim3(nwg), blk, 0, stream, M.dev(), v, nwg, rpw, nullptr, nullptr);
    }
    if (nparts) *nparts = 0;
    HIP_TRY(hipGetLastError());
    return MG_OK;
  }
  if (phase != 0 && !(v.nrhs == 1 && M.has_rc)) {
    if (phase == 1) {   // nothing is launched: no partial is written either (phase 2 computes the whole product)
      if (nparts) *nparts = 0;
      return MG_OK;
    }
    phase = 0;
  }
  if (phase == 2) {   // (v.sumsq, if set, points at the first free partial: the caller advanced it past phase 1's)
    if (nparts) *nparts = 0;
    if (M.rc_nexc > 0) {
      mgk::VecArgs ve = v;
      ve.d = v.d_full;
      const int nbx = (M.rc_nexc + mgk::BLK - 1) / mgk::BLK;
      hipLaunchKernelGGL((mgk::csr_rows_spmv<MODE>), dim3(nbx), blk, 0, stream, M.dev(), M.rc_exc.p, M.rc_nexc, ve, 0);
      HIP_TRY(hipGetLastError());
      if (nparts) *nparts = nbx;
    }
    return MG_OK;
  }
  if (v.nrhs == 1 && M.has_rc) {
    int nb_main;
    mgk::RowClassDev C = M.rcdev();
    if (phase == 1) C.nexc_inline = 0;    // the exception rows get their own launch (phase 2)
    const bool exc = C.nexc_inline > 0;   // a short list of exception rows rides in the last workgroup
    if (MODE == mgk::AXPBY && phase == 0 && marchr_ok(M, v)) {
      if (nparts) *nparts = 0;
      return launch_marchr(stream, M, v);
    }
    if (phase == 0 && march27_single_ok<MODE>(M, v)) {
      mgk::March2Args a{};
      a.x = v.x;
      a.b = v.b;
      a.t = v.y;
      if (nparts) *nparts = 0;
      return launch_march27<false, MODE == mgk::RESID ? mgk::RESID : mgk::SMOOTH>(stream, M, a);
    }
    if (march_ok(M, v)) {
      const mgk::MarchDev T = M.marchdev();
      const int SL = mgk::RM_C + 2 * M.rm_halo;
      const size_t lds = (size_t)mgk::RM_RING * (size_t)((SL + 3) & ~1) * sizeof(double) + mgk::RM_DICT_BYTES;
      nb_main = M.rm_nblocks;
      static bool lds_attr_set[3] = {false, false, false};
      if (!lds_attr_set[MODE]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&mgk::csr_rowclass_march_spmv<MODE, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&mgk::csr_rowclass_march_spmv<MODE, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
        (void)hipGetLastError();
        lds_attr_set[MODE] = true;
      }
      if (exc) hipLaunchKernelGGL((mgk::csr_rowclass_march_spmv<MODE, true>), dim3(nb_main), dim3(mgk::RM_C), lds, stream, C, v, T);
      else hipLaunchKernelGGL((mgk::csr_rowclass_march_spmv<MODE, false>), dim3(nb_main), dim3(mgk::RM_C), lds, stream, C, v, T);
    } else if (M.rc_tile && v.y != v.x) {   // (the staged variants read x workgroup-wide: never in place)
      const size_t lds = M.tile_lds_bytes();
      nb_main = M.rt_nblocks;
      static bool lds_attr_set[3] = {false, false, false};   // up to 80 KiB of dynamic LDS: lift the 64 KiB default once
      if (!lds_attr_set[MODE]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&mgk::csr_rowclass_tile_spmv<MODE, false, mgk::RT_CR>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&mgk::csr_rowclass_tile_spmv<MODE, true, mgk::RT_CR>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
        (void)hipGetLastError();
        lds_attr_set[MODE] = true;
      }
      if (M.rt_cr == 256) {
        if (exc) hipLaunchKernelGGL((mgk::csr_rowclass_tile_spmv<MODE, true, 256>), dim3(nb_main), dim3(256), lds, stream, C, v, M.tiledev());
        else hipLaunchKernelGGL((mgk::csr_rowclass_tile_spmv<MODE, false, 256>), dim3(nb_main), dim3(256), lds, stream, C, v, M.tiledev());
      } else {
        if (exc) hipLaunchKernelGGL((mgk::csr_rowclass_tile_spmv<MODE, true, mgk::RT_CR>), dim3(nb_main), dim3(mgk::RT_CR), lds, stream, C, v, M.tiledev());
        else hipLaunchKernelGGL((mgk::csr_rowclass_tile_spmv<MODE, false, mgk::RT_CR>), dim3(nb_main), dim3(mgk::RT_CR), lds, stream, C, v, M.tiledev());
      }
    } else if (M.rc_window && v.y != v.x) {
      nb_main = M.rw_blocks();
      const size_t lds = (size_t)M.rw_doubles * sizeof(double);
      if (exc) hipLaunchKernelGGL((mgk::csr_rowclass_window_spmv<MODE, true>), dim3(nb_main), blk, lds, stream, C, v, M.rw_meta.p, M.rw_lb.p, nb_main, (int)M.n_cols);
      else hipLaunchKernelGGL((mgk::csr_rowclass_window_spmv<MODE, false>), dim3(nb_main), blk, lds, stream, C, v, M.rw_meta.p, M.rw_lb.p, nb_main, (int)M.n_cols);
    } else if (MODE == mgk::AXPBY && M.rp_ok && v.y != v.x) {
      // a prolongation-shaped operator: the coarse windows of a workgroup's rows staged in LDS; exception rows (a sharded
      // level's rows that read halo columns) from the CSR arrays - behind it here, or as phase 2 behind the exchange
      const mgk::WinPDev T = M.winpdev();
      nb_main = T.nblocks;
      hipLaunchKernelGGL((mgk::csr_rowclass_winp_spmv<0>), dim3(nb_main), dim3(mgk::WP_T), M.winp_lds_bytes(), stream, C, v, T);
      if (M.rc_nexc > 0 && phase == 0) {
        mgk::VecArgs ve = v;
        ve.d = v.d_full;
        hipLaunchKernelGGL((mgk::csr_rows_spmv<MODE>), dim3((M.rc_nexc + mgk::BLK - 1) / mgk::BLK), blk, 0, stream, M.dev(), M.rc_exc.p, M.rc_nexc, ve, 0);
      }
      if (nparts) *nparts = 0;
      HIP_TRY(hipGetLastError());
      return MG_OK;
    } else if (M.rc_lane()) {
      nb_main = M.rc_blocks();
      mgk::LaneDev T;
      T.ncls = (int)M.rc_ncls;
      T.nent = (int)M.rc_entries;
      T.maxlen = M.rc_maxlen;
      T.nblocks = nb_main;
      // adjacent rows per lane (16-byte operand accesses) for operators whose classes alternate row by row (a
      // prolongation; measured on C2: P 115 -> 105 us, but R 59 -> 82 us), where the vectors are 16-byte aligned
      const bool pair = M.rc_pair && ((reinterpret_cast<uintptr_t>(v.y) | reinterpret_cast<uintptr_t>(v.b) |
                                       reinterpret_cast<uintptr_t>(v.d) | reinterpret_cast<uintptr_t>(v.xs)) & 15) == 0;
      if (pair) {
        if (exc) hipLaunchKernelGGL((mgk::csr_rowclass_lane_spmv<MODE, true, true>), dim3(nb_main), blk, 0, stream, C, v, T);
        else hipLaunchKernelGGL((mgk::csr_rowclass_lane_spmv<MODE, false, true>), dim3(nb_main), blk, 0, stream, C, v, T);
      } else {
        if (exc) hipLaunchKernelGGL((mgk::csr_rowclass_lane_spmv<MODE, true, false>), dim3(nb_main), blk, 0, stream, C, v, T);
        else hipLaunchKernelGGL((mgk::csr_rowclass_lane_spmv<MODE, false, false>), dim3(nb_main), blk, 0, stream, C, v, T);
      }
    } else {
      nb_main = M.rc_blocks();
      if (M.rc_pair) {
        if (exc) hipLaunchKernelGGL((mgk::csr_rowclass_spmv<MODE, true, true>), dim3(nb_main), blk, 0, stream, C, v);
        else hipLaunchKernelGGL((mgk::csr_rowclass_spmv<MODE, false, true>), dim3(nb_main), blk, 0, stream, C, v);
      } else {
        if (exc) hipLaunchKernelGGL((mgk::csr_rowclass_spmv<MODE, true, false>), dim3(nb_main), blk, 0, stream, C, v);
        else hipLaunchKernelGGL((mgk::csr_rowclass_spmv<MODE, false, false>), dim3(nb_main), blk, 0, stream, C, v);
      }
    }
    if (M.rc_nexc > mgk::BLK && phase == 0) {   // rows of rare classes, from the CSR arrays; their ||r||^2 partials follow the others
      mgk::VecArgs ve = v;
      ve.d = v.d_full;
      hipLaunchKernelGGL((mgk::csr_rows_spmv<MODE>), dim3(M.exc_blocks()), blk, 0, stream, M.dev(), M.rc_exc.p, M.rc_nexc, ve, nb_main);
    }
    if (nparts) *nparts = nb_main + (phase == 0 ? M.exc_blocks() : 0);
  } else if (v.nrhs == 1 && M.has_pat) {
    const bool dl = M.dict_entries <= mgk::DICT_LDS && M.npat < mgk::DICT_LDS;
    if (M.nt && dl) hipLaunchKernelGGL((mgk::csr_pattern_spmv<MODE, true, true>), grid, blk, 0, stream, M.dev(), M.patdev(), v);
    else if (M.nt) hipLaunchKernelGGL((mgk::csr_pattern_spmv<MODE, true, false>), grid, blk, 0, stream, M.dev(), M.patdev(), v);
    else if (dl) hipLaunchKernelGGL((mgk::csr_pattern_spmv<MODE, false, true>), grid, blk, 0, stream, M.dev(), M.patdev(), v);
    else hipLaunchKernelGGL((mgk::csr_pattern_spmv<MODE, false, false>), grid, blk, 0, stream, M.dev(), M.patdev(), v);
  } else if (v.nrhs == 1) {
    if (M.nt) hipLaunchKernelGGL((mgk::csr_stream_spmv<MODE, true>), grid, blk, 0, stream, M.dev(), v);
    else hipLaunchKernelGGL((mgk::csr_stream_spmv<MODE, false>), grid, blk, 0, stream, M.dev(), v);
  } else if (M.rc_lane_mm() && M.ln_blocks > 0 && M.ln_rows == lane_mm_rpl(M, v.nrhs) * (mgk::BLK / lane_mm_group(M, v.nrhs)) &&
             (!lane_mm_pairs(M, v.nrhs) || aligned16(v))) {
    mgk::LaneDev T;
    T.ncls = (int)M.rc_ncls;
    T.nent = (int)M.rc_entries;
    T.maxlen = M.rc_maxlen;
    T.nblocks = M.ln_blocks;
    const int G = lane_mm_group(M, v.nrhs);
    const int* sched = M.has_sched_ln ? M.sched_ln.p : nullptr;
    if (nparts) *nparts = lane_mm_pairs(M, v.nrhs) ? M.ln_blocks : 0;   // (only the paired form writes ||out||^2 partials)
    if (lane_mm_pairs(M, v.nrhs))   // two columns (16 bytes) per lane
      if (lane_mm_rpl(M, v.nrhs) == 3) hipLaunchKernelGGL((mgk::csr_rowclass_lane_spmm2<MODE, 3>), dim3(M.ln_blocks), blk, 0, stream, M.rcdev(), v, T, G, sched);
      else hipLaunchKernelGGL((mgk::csr_rowclass_lane_spmm2<MODE, 2>), dim3(M.ln_blocks), blk, 0, stream, M.rcdev(), v, T, G, sched);
    else
      hipLaunchKernelGGL((mgk::csr_rowclass_lane_spmm<MODE>), dim3(M.ln_blocks), blk, 0, stream, M.rcdev(), v, T, G, sched);
  } else {
    const int G = pow2_ge(v.nrhs);
    const dim3 grid_mm(M.nblocks_mm);
    if (M.nt) hipLaunchKernelGGL((mgk::csr_stream_spmm<MODE, true>), grid_mm, blk, 0, stream, M.dev_mm(), v, G);
    else hipLaunchKernelGGL((mgk::csr_stream_spmm<MODE, false>), grid_mm, blk, 0, stream, M.dev_mm(), v, G);
  }
  HIP_TRY(hipGetLastError());
  return MG_OK;
}

// The final sum of a four-stage pass's ||r||^2 partials that k_four_stage left to the next launch (h->dsum): as a launch of its own
int flush_deferred_sum(mg_hierarchy* h) {
  if (!h->dsum.on) return MG_OK;
  h->dsum.on = false;
  hipLaunchKernelGGL(mgk::sum_final_mirror, dim3(1), dim3(mgk::BLK), 0, h->play->stream, h->play->partial.p, h->dsum.np, h->play->scalar.p, h->dsum.host);
  HIP_TRY(hipGetLastError());
  if (h->dsum.ev) HIP_TRY(hipEventRecord(h->dsum.ev, h->play->stream));
  return MG_OK;
}
// y = alpha*M*x + beta*y
// d2 / y2 (optional, both or none; only where restrict_can_scale(M)): also y2 = d2 .* y
int k_spmv(mg_hierarchy* h, int level, int kind, const Csr& M, double alpha, const double* x,
           double beta, double* y, const double* d2 = nullptr, double* y2 = nullptr) {
  if (h->dsum.on) {
    // the fine restriction behind a four-stage pass: its grid takes one more workgroup, which adds up the pass's partial sums
    if (kind == MG_K_RESTRICT && level == 0 && h->play->nrhs == 1 && M.waver_ok && !M.wide && alpha == 1.0 && beta == 0.0 && y && y != x && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && !h->prof && !h->capturing) {
      const long long waves = (M.n_rows + 61) / 62;
      h->dsum.on = false;
      hipLaunchKernelGGL(mgk::grid_wave_restrict, dim3((unsigned)((waves + 3) / 4 + 1)), dim3(256), 0, h->play->stream, M.smr, M.waver_scale, x, y,
                         y2 ? d2 : nullptr, y2, mgk::FinalSum{h->play->partial.p, h->dsum.np, h->play->scalar.p, h->dsum.host});
      HIP_TRY(hipGetLastError());
      if (h->dsum.ev) HIP_TRY(hipEventRecord(h->dsum.ev, h->play->stream));
      return MG_OK;
    }
    MG_TRY(flush_deferred_sum(h));
  }
  mgk::VecArgs v{};
  v.x = x;
  v.y = y;
  v.alpha = alpha;
  v.beta = beta;
  v.nrhs = (int)h->play->nrhs;
  v.d_full = d2;
  v.y2 = y2;
  const double extra = y2 ? 16.0 * (double)M.n_rows : 0.0;
  ProfScope ps(h, level, kind, spmv_bytes(M, h->play->nrhs, beta != 0.0, false) + extra, moved_bytes(M, h->play->nrhs, beta != 0.0, false) + extra);
  return launch_csr<mgk::AXPBY>(h->play->stream, M, v);
}
// Is the product with M served, for one right-hand side, by a kernel that can write d.*out too (csr_rowclass_lane_spmv, or the
// streaming kernels csr_pattern_spmv / csr_stream_spmv for operators without row classes)?
bool restrict_can_scale(const mg_hierarchy* h, const Csr& M) {
  if (h->play->nrhs != 1 || h->opt.no_restrict_scale) return false;
  if (M.smr_use() || M.waver_ok) return true;
  if (!M.has_rc) return M.max_row_nnz <= mgk::CHUNK - 2;   // the streaming kernels (pattern-coded or plain CSR), short rows: epilogue output
  if (M.rc_marchr && !M.opt.no_marchr) return true;
  return M.rc_nexc == 0 && !M.rc_march && !M.rc_tile && !M.rc_window && !M.rp_ok && M.rc_lane();
}
// out = b - A*x
int k_residual(mg_hierarchy* h, int level, const Csr& A, const double* b, const double* x,
               double* out) {
  mgk::VecArgs v{};
  v.x = x;
  v.y = out;
  v.b = b;
  v.nrhs = (int)h->play->nrhs;
  ProfScope ps(h, level, MG_K_RESIDUAL, spmv_bytes(A, h->play->nrhs, true, false), moved_bytes(A, h->play->nrhs, true, false));
  return launch_csr<mgk::RESID>(h->play->stream, A, v);
}
// ---- two launches of a small level as one (mg_small.hpp: grid27_small_resid_restrict / grid27_small_prolong_smooth) -----------------
// the level's A has position-class records whose relaxPrec is the level's, its transfers are the verified arithmetic forms of an
// ORDINARY grid pair (not an embedded one), one right-hand side (the caller keeps sharded levels out)
bool small_fuse_rr_ok(const mg_hierarchy* h, int level) {
  if (h->opt.no_small_fuse || h->play->nrhs != 1 || level + 1 >= (int)h->nlevels) return false;
  const Level& L = h->lev[(size_t)level];
  const Csr &A = L.A, &R = L.R;
  if (!A.sm_ok || !R.waver_ok || R.waver_scale == 0.0) return false;
  const mgk::SmallRDev& T = R.smr;
  return T.o1 == 0 && T.o2 == 0 && T.o3 == 0 && T.m1 == T.nc1 && T.m2 == T.nc2 && T.m3 == T.nc3 && T.nf1 == A.sm.n1 && T.nf2 == A.sm.n2 && T.nf3 == A.sm.n3 &&
         T.nf1 == 2 * T.nc1 - 1 && T.nf2 == 2 * T.nc2 - 1 && T.nf3 == 2 * T.nc3 - 1;
}
bool small_fuse_ps_ok(const mg_hierarchy* h, int level) {
  if (h->opt.no_small_fuse || h->play->nrhs != 1 || level + 1 >= (int)h->nlevels || h->relax_type != 0) return false;
  const Level& L = h->lev[(size_t)level];
  const Csr &A = L.A, &P = L.P;
  if (!A.sm_ok || !A.sm_d_bound || A.sm_d_bound != L.d.p || !(P.cellp_ok || P.smp_ok)) return false;
  const mgk::SmallPDev& T = P.smp;
  return T.o1 == 0 && T.o2 == 0 && T.o3 == 0 && T.m1 == T.nc1 && T.m2 == T.nc2 && T.m3 == T.nc3 && T.nf1 == A.sm.n1 && T.nf2 == A.sm.n2 && T.nf3 == A.sm.n3;
}
// bc = R (b - A x) [, y2 = d2 .* bc]: the residual lives in LDS only
int k_small_resid_restrict(mg_hierarchy* h, int level, const double* b, const double* x, double* bc, const double* d2, double* y2) {
  const Level& L = h->lev[(size_t)level];
  const mgk::SmallRDev& T = L.R.smr;
  const double bytes = 8.0 * (2.0 * (double)L.A.n_rows + (double)L.R.n_rows * (y2 ? 3.0 : 1.0));
  ProfScope ps(h, level, MG_K_RESTRICT, bytes, bytes);
  const unsigned nb = (unsigned)(((T.nc1 + mgk::SRR_CT - 1) / mgk::SRR_CT) * ((T.nc2 + mgk::SRR_CT - 1) / mgk::SRR_CT) * ((T.nc3 + mgk::SRR_CT - 1) / mgk::SRR_CT));
  hipLaunchKernelGGL(mgk::grid27_small_resid_restrict, dim3(nb), dim3(256), 0, h->play->stream, L.A.sm, T, L.R.waver_scale, x, b, bc, y2 ? d2 : nullptr, y2);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
// y = (x + P xc) + d.*(b - A (x + P xc)): the corrected x lives in LDS only
int k_small_prolong_smooth(mg_hierarchy* h, int level, const double* xc, const double* x, const double* b, double* y) {
  const Level& L = h->lev[(size_t)level];
  const mgk::Small27Dev& A = L.A.sm;
  const double bytes = 8.0 * (3.0 * (double)L.A.n_rows + (double)L.P.n_cols);
  ProfScope ps(h, level, MG_K_SMOOTH_PROLONG, bytes, bytes);
  const unsigned nb = (unsigned)(((A.n1 + mgk::SPS_TX - 1) / mgk::SPS_TX) * ((A.n2 + mgk::SPS_TY - 1) / mgk::SPS_TY) * ((A.n3 + mgk::SPS_TZ - 1) / mgk::SPS_TZ));
  hipLaunchKernelGGL(mgk::grid27_small_prolong_smooth, dim3(nb), dim3(256), 0, h->play->stream, A, L.P.smp, xc, x, b, y);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
int k_sumsq(mg_hierarchy* h, const double* x, long long len);
// out = b - A*x and h->play->scalar = ||out||^2 in the same pass (nrhs == 1); falls back to two kernels for blocks
// xnext (optional): also write x + d.*(b - A x), the first damped-Jacobi update of the next cycle, when the kernel
// that serves A can do it (plane-tile row-class kernel, level's own relaxPrec); *xnext_done reports whether it was.
// r_dead: the caller will not read `out` when xnext was written (the solve loop: the next cycle starts from xnext and
// recomputes its own residual), so the store of r is skipped as well.
int k_residual_sumsq(mg_hierarchy* h, int level, const Csr& A, const double* b, const double* x, double* out,
                     double* xnext = nullptr, bool* xnext_done = nullptr, bool r_dead = false) {
  if (xnext_done) *xnext_done = false;
  mgk::VecArgs v{};
  v.x = x;
  v.y = out;
  v.b = b;
  v.nrhs = (int)h->play->nrhs;
  if (h->play->nrhs != 1) {
    // block right-hand sides: the paired-column lane SpMM writes ||r||^2 partials and, optionally, x + d.*r
    const bool fused = A.rc_lane_mm() && A.ln_blocks > 0 && lane_mm_pairs(A, h->play->nrhs) &&
                       A.ln_rows == lane_mm_rpl(A, h->play->nrhs) * (mgk::BLK / lane_mm_group(A, h->play->nrhs)) && (size_t)A.ln_blocks <= h->play->partial.n;
    mgk::VecArgs t = v;
    t.xs = x;
    if (xnext) t.y2 = xnext;
    if (!fused || !aligned16(t) || (xnext && (reinterpret_cast<uintptr_t>(xnext) & 15u))) {
      MG_TRY(k_residual(h, level, A, b, x, out));
      return k_sumsq(h, out, A.n_rows * h->play->nrhs);
    }
    v.sumsq = h->play->partial.p;
    if (xnext && out != x && xnext != x && h->relax_type == 0 && &A == &h->lev[(size_t)level].A && !h->opt.no_fused_next) {
      v.y2 = xnext;
      if (r_dead) v.y = nullptr;
      v.xs = x;
      v.d = v.d_full = h->lev[(size_t)level].d.p;
      if (xnext_done) *xnext_done = true;
    }
    int nb1 = 0;
    {
      const double vec = 8.0 * (double)A.n_rows * (double)h->play->nrhs;
      ProfScope ps(h, level, MG_K_RESIDUAL, spmv_bytes(A, h->play->nrhs, true, false) + ((v.y2 && v.y) ? vec : 0.0),
                   moved_bytes(A, h->play->nrhs, true, false) - (v.y ? 0.0 : vec) + (v.y2 ? vec : 0.0));
      MG_TRY(launch_csr<mgk::RESID>(h->play->stream, A, v, &nb1));
    }
    ProfScope ps2(h, level, MG_K_NORM, 8.0 * (double)nb1, 8.0 * (double)nb1);
    const int nb2 = std::min(256, (nb1 + mgk::BLK - 1) / mgk::BLK);
    hipLaunchKernelGGL(mgk::sum_partial, dim3(nb2), dim3(mgk::BLK), 0, h->play->stream, h->play->partial.p, (long long)nb1, h->play->partial2.p);
    launch_sum_final(h, h->play->partial2.p, nb2);
    HIP_TRY(hipGetLastError());
    return MG_OK;
  }
  if ((size_t)std::max(A.blocks1(), A.nblocks) > h->play->partial.n) {
    MG_TRY(k_residual(h, level, A, b, x, out));
    return k_sumsq(h, out, A.n_rows * h->play->nrhs);
  }
  v.sumsq = h->play->partial.p;
  // the LDS-staged row-class kernels (march, tile) have x, r and the class's relaxPrec at hand: second output
  if (xnext && A.has_rc && (A.rc_tile || march_ok(A, v)) && A.rc_nexc == 0 && out != x && xnext != x && h->relax_type == 0 &&
      &A == &h->lev[(size_t)level].A && !h->opt.no_fused_next) {
    v.y2 = xnext;
    if (r_dead) v.y = nullptr;
    v.xs = x;
    v.d = A.rc_has_d ? nullptr : h->lev[(size_t)level].d.p;
    v.d_full = h->lev[(size_t)level].d.p;
    if (xnext_done) *xnext_done = true;
  }
  int nb1 = 0;
  {
    ProfScope ps(h, level, MG_K_RESIDUAL, spmv_bytes(A, 1, true, false) + ((v.y2 && v.y) ? 8.0 * (double)A.n_rows : 0.0),
                 moved_bytes(A, 1, true, false) - (v.y ? 0.0 : 8.0 * (double)A.n_rows) + (v.y2 ? 8.0 * (double)A.n_rows : 0.0));
    MG_TRY(launch_csr<mgk::RESID>(h->play->stream, A, v, &nb1));
  }
  ProfScope ps2(h, level, MG_K_NORM, 8.0 * (double)nb1, 8.0 * (double)nb1);
  const int nb2 = std::min(256, (nb1 + mgk::BLK - 1) / mgk::BLK);
  hipLaunchKernelGGL(mgk::sum_partial, dim3(nb2), dim3(mgk::BLK), 0, h->play->stream, h->play->partial.p, (long long)nb1, h->play->partial2.p);
  launch_sum_final(h, h->play->partial2.p, nb2);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
int scalar_sync(mg_hierarchy* h, double* out);
int scalar_wait(mg_hierarchy* h);

// out = x + d.*(b - A*x)
int k_smooth(mg_hierarchy* h, int level, const Csr& A, const double* d, const double* b,
             const double* x, double* out) {
  mgk::VecArgs v{};
  v.x = x;
  v.xs = x;
  v.y = out;
  v.b = b;
  v.d = d;
  v.d_full = d;
  // the level's own relaxPrec, constant per row class: read from the dictionary instead of streamed (rc_d)
  if (h->play->nrhs == 1 && A.has_rc && A.rc_has_d && d == h->lev[(size_t)level].d.p && &A == &h->lev[(size_t)level].A) v.d = nullptr;
  if (h->play->nrhs == 1 && A.sm_use() && A.sm_d_bound == d && d == h->lev[(size_t)level].d.p && &A == &h->lev[(size_t)level].A) v.d = nullptr;
  v.nrhs = (int)h->play->nrhs;
  ProfScope ps(h, level, MG_K_SMOOTH, spmv_bytes(A, h->play->nrhs, true, true), moved_bytes(A, h->play->nrhs, true, true, v.d == nullptr));
  return launch_csr<mgk::SMOOTH>(h->play->stream, A, v);
}
// One sweep and the residual of its result in one pass (csr_rowclass_march2_spmv):
//   t = x + d.*(b - A x) ;  r = b - A t  [; xn = t + d.*r ; ||r||^2 partials]
// for the level's own A with its own relaxPrec read from the class dictionary.  x, t, r, xn: four different buffers.
bool march2_ok(const mg_hierarchy* h, int level, const double* x, const double* t, const double* r, const double* xn) {
  const Level& L = h->lev[(size_t)level];
  if (h->play->nrhs != 1 || h->relax_type != 0) return false;
  if (L.A.rm3_var && L.A.rc_march3) {        // band form: values and relaxPrec are streamed per row
    if (!L.relax_set) return false;
  } else {
    if (!L.A.has_rc || !L.A.rc_has_d || L.A.rc_nexc != 0) return false;
    if (!(L.A.rc_march && L.A.rc_march2) && !L.A.rc_march3) {
      // the 27-point form serves the cycle's pair only: t and r out, nothing else
      if (!(L.A.rc_march27 && !L.A.opt.no_march27 && t && r && !xn)) return false;
    }
    if (L.A.d_bound != L.d.p) return false;   // the dictionary's relaxPrec is this level's
  }
  if ((t && (x == t || t == r || t == xn)) || x == r || x == xn || (r && r == xn)) return false;   // (t, r, xn: each optional)
  return (reinterpret_cast<uintptr_t>(x) & 15) == 0;
}
// the 2-D tile form (csr_rowclass_march3_spmv): template arguments from what is wanted
// (12 >= stores per lane and iteration: K1 <= 4 rows x 3 outputs; 32 slabs shared by all workgroups; 1024 lanes)
constexpr size_t M3_SINK_DOUBLES = (size_t)12 * 32 * 1024;
// > 64 KB of dynamic LDS needs the function attribute - per DEVICE: one bit per device id, set on the first launch there
static int big_lds_attr(const void* fn, std::atomic<unsigned long long>& done, size_t bytes) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  const unsigned long long bit = 1ULL << (dev & 63);
  if (done.load(std::memory_order_acquire) & bit) return MG_OK;
  HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  done.fetch_or(bit, std::memory_order_release);
  return MG_OK;
}
template <bool ZERO, int OUT, int NT, int K1, bool VAR = false>
int launch_march3(hipStream_t stream, const Csr& A, const mgk::March2Args& a) {
  auto* fn = &mgk::csr_rowclass_march3_spmv<ZERO, OUT, NT, K1, RM3_NPM, VAR>;
  static std::atomic<unsigned long long> attr_done{0};
  MG_TRY(big_lds_attr(reinterpret_cast<const void*>(fn), attr_done));
  mgk::RowClassDev C = A.rcdev();
  if (VAR) {
    C = mgk::RowClassDev{};
    C.n_rows = (int)A.n_rows;
  }
  hipLaunchKernelGGL(fn, dim3((unsigned)A.rm3.nblocks), dim3(NT), A.rm3_lds, stream, C, a, A.rm3);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
template <bool ZERO, int OUT>
int launch_march3_k(hipStream_t stream, const Csr& A, const mgk::March2Args& a) {
  if (A.rm3_var) return A.rm3_k1 == 2 ? launch_march3<ZERO, OUT, 512, 2, true>(stream, A, a) : launch_march3<ZERO, OUT, 512, 3, true>(stream, A, a);
  if (A.rm3_nt == 768) return A.rm3_k1 == 3 ? launch_march3<ZERO, OUT, 768, 3>(stream, A, a) : launch_march3<ZERO, OUT, 768, 4>(stream, A, a);
  return A.rm3_k1 == 2 ? launch_march3<ZERO, OUT, 1024, 2>(stream, A, a) : launch_march3<ZERO, OUT, 1024, 3>(stream, A, a);
}
// dispatch on (from_zero, outputs); `scratch` (n_rows doubles, may be null when t and one of r / xn are given in one of the
// instantiated combinations) takes the outputs nobody asked for
int launch_march3_any(hipStream_t stream, const Csr& A, mgk::March2Args a, bool from_zero, double* scratch) {
  int o = (a.r ? 1 : 0) | (a.xn ? 2 : 0) | (a.t ? 4 : 0);
  if (!(o == 5 || o == 2 || o == 6 || o == 7)) {   // (t, r) cycle; (xn) solve loop, iterate dead; (t, xn) its last step; all
    if (!scratch) return fail(MG_ERR_STATE, "this combination of outputs needs a scratch vector");
    if (!a.t) a.t = scratch;      // (one scratch vector takes every output nobody asked for: written, never read)
    if (!a.r) a.r = scratch;
    if (!a.xn) a.xn = scratch;
    o = 7;
  }
  if (from_zero) return o == 5 ? launch_march3_k<true, 5>(stream, A, a) : o == 2 ? launch_march3_k<true, 2>(stream, A, a) : o == 6 ? launch_march3_k<true, 6>(stream, A, a) : launch_march3_k<true, 7>(stream, A, a);
  return o == 5 ? launch_march3_k<false, 5>(stream, A, a) : o == 2 ? launch_march3_k<false, 2>(stream, A, a) : o == 6 ? launch_march3_k<false, 6>(stream, A, a) : launch_march3_k<false, 7>(stream, A, a);
}
int k_smooth_residual3(mg_hierarchy* h, int level, const Csr& A, const mgk::March2Args& a_in, bool from_zero) {
  mgk::March2Args a = a_in;
  const int nb1 = A.rm3.nblocks;
  if (h->m3sink.n < M3_SINK_DOUBLES) return fail(MG_ERR_STATE, "the store sink of the tile-form pass is missing (mg_finalize allocates it)");
  a.sink = h->m3sink.p;
  a.d = h->lev[(size_t)level].d.p;
  if (a.sumsq && (size_t)nb1 > h->play->partial.n) return fail(MG_ERR_STATE, "partial-sum buffer too small for the fused sweep + residual");
  const double n8 = 8.0 * (double)A.n_rows;
  {
    // moved: no class-id stream in this form (the ids come from the product map) - the class records, the index maps, x and b
    // in, the outputs asked for out
    // (band form: + the 7 planar value arrays - 4 where the symmetric reads serve the operator - and relaxPrec, once for both stages)
    const double tables = (double)(A.rm3_var ? A.band_ncls : A.rc_ncls) * 88.0 + 2.0 * (double)(A.rm3.n1 + A.rm3.n2 + A.rm3.nplanes + A.rm3.ntab) +
                          (A.rm3_var ? 8.0 * (double)((A.band_sym ? 4 : mgk::RM3_NIP + 2) + 1) * (double)A.n_rows : 0.0);
    ProfScope ps(h, level, a.sumsq ? MG_K_SMOOTH_RESIDUAL_NORM : MG_K_SMOOTH_RESIDUAL, spmv_bytes(A, 1, true, true) + spmv_bytes(A, 1, true, false) + (a.xn && a.r ? n8 : 0.0),
                 tables + n8 * (2.0 + (a.t ? 1.0 : 0.0) + (a.r ? 1.0 : 0.0) + (a.xn ? 1.0 : 0.0)));
    // the combinations the cycle and the solve loop use are instantiated exactly; anything else (the test entry point) runs
    // the all-outputs kernel with the missing vectors pointed at a scratch vector of the level
    const int o = (a.r ? 1 : 0) | (a.xn ? 2 : 0) | (a.t ? 4 : 0);
    double* scratch = nullptr;
    if (!(o == 5 || o == 2 || o == 6 || o == 7)) {
      Level& L = h->lev[(size_t)level];
      if (L.x3.n != (size_t)A.n_rows) MG_TRY(L.x3.alloc((size_t)A.n_rows));
      scratch = L.x3.p;
    }
    MG_TRY(launch_march3_any(h->play->stream, A, a, from_zero, scratch));
  }
  if (a.sumsq) {
    ProfScope ps2(h, level, MG_K_NORM, 8.0 * (double)nb1, 8.0 * (double)nb1);
    launch_sum_final(h, h->play->partial.p, nb1);
    HIP_TRY(hipGetLastError());
  }
  return MG_OK;
}
// from_zero: the sweep's input is x1 = d.*b (the level is entered with x = 0): x is not read, no dscale launch is needed
int k_smooth_residual(mg_hierarchy* h, int level, const double* b, const double* x, double* t, double* r, double* xn,
                      bool want_sumsq, bool from_zero = false) {
  const Csr& A = h->lev[(size_t)level].A;
  mgk::March2Args a{};
  a.x = x;
  a.b = b;
  a.t = t;
  a.r = r;
  a.xn = xn;
  a.sumsq = want_sumsq ? h->play->partial.p : nullptr;
  if (A.rc_march3) return k_smooth_residual3(h, level, A, a, from_zero);
  if (A.rc_march27 && !A.opt.no_march27 && t && r && !xn && !want_sumsq && (!from_zero || !A.opt.no_march27_zero)) {
    const double n8 = 8.0 * (double)A.n_rows;
    const double tables = (double)A.rc_ncls * 224.0 + 2.0 * (double)(A.rm27[1].n1 + A.rm27[1].n2 + A.rm27[1].nplanes + A.rm27[1].ntab);
    ProfScope ps(h, level, MG_K_SMOOTH_RESIDUAL, spmv_bytes(A, 1, true, true) + spmv_bytes(A, 1, true, false), tables + (from_zero ? 3.0 : 4.0) * n8);
    if (from_zero) return launch_march27<true, mgk::SMOOTH, true>(h->play->stream, A, a);   // x1 = d.*b inside the walk: x is not read
    return launch_march27<true, mgk::SMOOTH>(h->play->stream, A, a);
  }
  if (!(A.rc_march && A.rc_march2)) return fail(MG_ERR_UNSUPPORTED, "this combination of outputs is not served by a two-stage pass on level %d", level + 1);
  mgk::MarchDev T = A.marchdev();
  T.nblocks = A.rm2_nblocks;
  if (want_sumsq && (size_t)T.nblocks > h->play->partial.n) return fail(MG_ERR_STATE, "partial-sum buffer too small for the fused sweep + residual");
  const size_t lds = march2_lds_bytes(A.rm_halo);
  static bool lds_attr_set = false;
  if (!lds_attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&mgk::csr_rowclass_march2_spmv<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&mgk::csr_rowclass_march2_spmv<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256);
    (void)hipGetLastError();
    lds_attr_set = true;
  }
  const double n8 = 8.0 * (double)A.n_rows;
  {
    // algorithmic: the two products; moved: class ids + x + b in, t and r (and/or xn) out
    ProfScope ps(h, level, want_sumsq ? MG_K_SMOOTH_RESIDUAL_NORM : MG_K_SMOOTH_RESIDUAL, spmv_bytes(A, 1, true, true) + spmv_bytes(A, 1, true, false) + (xn && r ? n8 : 0.0),
                 format_bytes(A, 1) + n8 * (2.0 + (t ? 1.0 : 0.0) + (r ? 1.0 : 0.0) + (xn ? 1.0 : 0.0)));
    if (from_zero) hipLaunchKernelGGL((mgk::csr_rowclass_march2_spmv<true>), dim3(T.nblocks), dim3(mgk::RM_C), lds, h->play->stream, A.rcdev(), a, T);
    else hipLaunchKernelGGL((mgk::csr_rowclass_march2_spmv<false>), dim3(T.nblocks), dim3(mgk::RM_C), lds, h->play->stream, A.rcdev(), a, T);
    HIP_TRY(hipGetLastError());
  }
  if (want_sumsq) {   // one partial per workgroup (<= one per CU): a single-workgroup final sum
    const int nb1 = T.nblocks;
    ProfScope ps2(h, level, MG_K_NORM, 8.0 * (double)nb1, 8.0 * (double)nb1);
    launch_sum_final(h, h->play->partial.p, nb1);
    HIP_TRY(hipGetLastError());
  }
  return MG_OK;
}
// The solve loop's two fine-level passes across the stopping test as ONE four-stage pass (csr_rowclass_march4_spmv):
//   t = x + d.*(b - A x) ; r = b - A t ; ||r||^2 ; xn = t + d.*r ; tp = xn + d.*(b - A xn) ; rp = b - A tp
// x, tp, rp: three different buffers; the iterate t is not stored (the caller re-creates it from x if the loop stops).
template <int NT, int K1, int NPM, int PITCH>
int launch_march4_p(hipStream_t stream, const Csr& A, const mgk::March2Args& a, const mgk::March4Dev& T) {
  auto* fn = &mgk::csr_rowclass_march4_spmv<NT, K1, NPM, PITCH>;
  static std::atomic<unsigned long long> attr_done{0};
  MG_TRY(big_lds_attr(reinterpret_cast<const void*>(fn), attr_done));
  hipLaunchKernelGGL(fn, dim3((unsigned)T.nblocks), dim3(NT), A.rm4_lds, stream, A.rcdev(), a, T);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
// (the slab pitch is a template argument: LDS line offsets as immediates; build_march4 pads a tile's lines to one of these)
// T: A.rm4, or a copy of it whose ||r||^2 box is the owned box of a rank (ghost-layer form)
template <int NT, int K1, int NPM>
int launch_march4(hipStream_t stream, const Csr& A, const mgk::March2Args& a, const mgk::March4Dev& T) {
  switch (T.pitch) {
    case 48: return launch_march4_p<NT, K1, NPM, 48>(stream, A, a, T);
    case 64: return launch_march4_p<NT, K1, NPM, 64>(stream, A, a, T);
    case 80: return launch_march4_p<NT, K1, NPM, 80>(stream, A, a, T);
    default: return fail(MG_ERR_STATE, "four-stage pass: no kernel for a slab pitch of %d", T.pitch);
  }
}
bool march4_ok(const mg_hierarchy* h, int level, const double* x, const double* tp, const double* rp) {
  const Level& L = h->lev[(size_t)level];
  if (h->play->nrhs != 1 || h->relax_type != 0 || h->opt.no_march4) return false;
  if (!L.A.rc_march4 || !L.A.has_rc || !L.A.rc_has_d || L.A.rc_nexc != 0 || L.A.d_bound != L.d.p) return false;
  if (std::max<long long>(1, L.npre) != 2) return false;   // (xn is the input of the LAST pre-smoothing sweep)
  if (x == tp || x == rp || tp == rp) return false;
  return (reinterpret_cast<uintptr_t>(x) & 15) == 0;
}
// The parts of march4_ok / march2_ok / restrict_can_scale that do not depend on the buffers of a call (the level's operator formats,
// smoother and sweep counts): what mg_ghost_finalize lets the ranks of a sharded run agree on.
bool march4_ok_static(const mg_hierarchy* h, int level) {
  const Level& L = h->lev[(size_t)level];
  if (h->relax_type != 0 || h->opt.no_march4) return false;
  if (!L.A.rc_march4 || !L.A.has_rc || !L.A.rc_has_d || L.A.rc_nexc != 0 || L.A.d_bound != L.d.p) return false;
  return std::max<long long>(1, L.npre) == 2;
}
bool march2_ok_static(const mg_hierarchy* h, int level) {
  const Level& L = h->lev[(size_t)level];
  if (h->relax_type != 0) return false;
  if (L.A.rm3_var && L.A.rc_march3) return L.relax_set;
  if (!L.A.has_rc || !L.A.rc_has_d || L.A.rc_nexc != 0) return false;
  if (!(L.A.rc_march && L.A.rc_march2) && !L.A.rc_march3 && !(L.A.rc_march27 && !L.A.opt.no_march27)) return false;
  return L.A.d_bound == L.d.p;
}
// the fused sweep + residual of this operator has a from-zero form (x1 = d.*b formed inside the pass)
bool zero_form_static(const Csr& A) {
  return A.rc_march3 || (A.rc_march && A.rc_march2) || (A.rc_march27 && !A.opt.no_march27 && !A.opt.no_march27_zero);
}
inline bool gh_agree_zero(const mg_hierarchy* h, int l);   // (mg_ghost.inc)
inline bool gh_agree2(const mg_hierarchy* h, int l);
// will a cycle entering level `level` with x = 0 form x1 = d.*b inside its first fused pass?  (what cycle_level decides, from what is
// known before the launch: the restriction INTO the level then writes no x1)
bool from_zero_static(const mg_hierarchy* h, int level) {
  const Level& L = h->lev[(size_t)level];
  return h->play->nrhs == 1 && std::max<long long>(1, L.npre) == 2 && !h->opt.no_march2_zero && march2_ok_static(h, level) && zero_form_static(L.A) &&
         gh_agree_zero(h, level) && gh_agree2(h, level);
}
bool restrict_can_scale_static(const mg_hierarchy* h, const Csr& M) {
  if (h->opt.no_restrict_scale) return false;
  if (M.smr_use() || M.waver_ok) return true;
  if (!M.has_rc) return M.max_row_nnz <= mgk::CHUNK - 2;
  if (M.rc_marchr && !M.opt.no_marchr) return true;
  return M.rc_nexc == 0 && !M.rc_march && !M.rc_tile && !M.rc_window && !M.rp_ok && M.rc_lane();
}
// defer_ev (the solve loop; with host_slot): the final sum of the partials may be left to the NEXT launch - the fine restriction of the
// cycle that follows (k_spmv) - which then records defer_ev; *deferred tells the caller whether it was (else the caller records it)
int k_four_stage(mg_hierarchy* h, int level, const double* b, const double* x, double* tp, double* rp, double* host_slot = nullptr,
                 hipEvent_t defer_ev = nullptr, bool* deferred = nullptr) {
  MG_TRY(flush_deferred_sum(h));   // (a previous pass's sum nobody picked up: it reads the partials this pass overwrites)
  if (deferred) *deferred = false;
  const Csr& A = h->lev[(size_t)level].A;
  mgk::March2Args a{};
  a.x = x;
  a.b = b;
  a.t = tp;
  a.r = rp;
  a.sumsq = h->play->partial.p;
  if (h->m3sink.n < M3_SINK_DOUBLES) return fail(MG_ERR_STATE, "the store sink of the tile-form pass is missing (mg_finalize allocates it)");
  a.sink = h->m3sink.p;
  a.d = h->lev[(size_t)level].d.p;
  const int nb1 = A.rm4.nblocks;
  if ((size_t)nb1 > h->play->partial.n) return fail(MG_ERR_STATE, "partial-sum buffer too small for the four-stage pass");
  const double n8 = 8.0 * (double)A.n_rows;
  {
    const double tables = (double)A.rc_ncls * 88.0 + 2.0 * (double)(A.rm4.n1 + A.rm4.n2 + A.rm4.nplanes + A.rm4.ntab);
    // algorithmic: four products with A (two fused sweeps, two residuals); moved: x, b in, t' and r' out
    ProfScope ps(h, level, MG_K_FOUR_STAGE, 2.0 * (spmv_bytes(A, 1, true, true) + spmv_bytes(A, 1, true, false)), tables + 4.0 * n8);
    mgk::March4Dev T = A.rm4;
    gh_own_box(h, level, &T.oxl, &T.oxh, &T.oyl, &T.oyh, &T.ozl, &T.ozh);   // (ghost-layer form: ||r||^2 over this rank's owned rows)
    if (A.rm4_nt == 1024) MG_TRY((launch_march4<1024, 2, 2>(h->play->stream, A, a, T)));
    else if (A.rm4_nt == 768 && A.rm4_k1 == 3) MG_TRY((launch_march4<768, 3, 2>(h->play->stream, A, a, T)));
    else if (A.rm4_nt == 768) MG_TRY((launch_march4<768, 4, 3>(h->play->stream, A, a, T)));
    else MG_TRY((launch_march4<512, 4, 3>(h->play->stream, A, a, T)));
  }
  ProfScope ps2(h, level, MG_K_NORM, 8.0 * (double)nb1, 8.0 * (double)nb1);
  if (gh_global_scalars(h)) {         // sharded: the ranks' sums are added before the host sees the norm (RCCL on the stream; plug-in: when it is read)
    hipLaunchKernelGGL(mgk::sum_final, dim3(1), dim3(mgk::BLK), 0, h->play->stream, h->play->partial.p, nb1, h->play->scalar.p);
    HIP_TRY(hipGetLastError());
    MG_TRY(gh_scalar_to_slot(h, host_slot ? host_slot : h->h_scalar));
    h->play->scalar_mirrored = true;
  } else if (host_slot && !h->capturing && deferred && !h->prof && !h->opt.no_defer_sum) {
    h->dsum.on = true;
    h->dsum.np = nb1;
    h->dsum.host = host_slot;
    h->dsum.ev = defer_ev;
    *deferred = true;
  } else if (host_slot && !h->capturing) {   // (the pipelined stopping test: a pinned slot per step in flight)
    hipLaunchKernelGGL(mgk::sum_final_mirror, dim3(1), dim3(mgk::BLK), 0, h->play->stream, h->play->partial.p, nb1, h->play->scalar.p, host_slot);
  } else {
    launch_sum_final(h, h->play->partial.p, nb1);
  }
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
int k_dscale(mg_hierarchy* h, int level, const double* d, const double* b, double* x, long long n) {
  ProfScope ps(h, level, MG_K_DSCALE, 8.0 * (double)n * (1.0 + 2.0 * (double)h->play->nrhs));
  hipLaunchKernelGGL(mgk::dscale_kernel, dim3(grid_for(n * h->play->nrhs / 2 + 1)), dim3(mgk::BLK), 0,
                     h->play->stream, d, b, x, n, (int)h->play->nrhs);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
// xout = x + d.*r (first sweep when r = b - A x is already known)
int k_xpdr(mg_hierarchy* h, int level, const double* x, const double* d, const double* r, double* xout,
           long long n) {
  ProfScope ps(h, level, MG_K_DSCALE, 8.0 * (double)n * (1.0 + 3.0 * (double)h->play->nrhs));
  const Csr& A = h->lev[(size_t)level].A;
  if (h->play->nrhs == 1 && A.has_rc && A.rc_has_d && d == h->lev[(size_t)level].d.p && n == A.n_rows) {
    // the level's relaxPrec is constant per row class: stream the 2-byte class ids instead of d
    hipLaunchKernelGGL(mgk::xpdr_cls_kernel, dim3(grid_for(n / 2 + 1)), dim3(mgk::BLK), 0, h->play->stream, x, A.rc_cls.p,
                       A.rc_d.p, d, r, xout, n);
    HIP_TRY(hipGetLastError());
    return MG_OK;
  }
  hipLaunchKernelGGL(mgk::xpdr_kernel, dim3(grid_for(n * h->play->nrhs / 2 + 1)), dim3(mgk::BLK), 0,
                     h->play->stream, x, d, r, xout, n, (int)h->play->nrhs);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
int k_fill(mg_hierarchy* h, double* x, long long n, double val) {
  hipLaunchKernelGGL(mgk::fill_kernel, dim3(grid_for(n)), dim3(mgk::BLK), 0, h->play->stream, x, n, val);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
int fgmres_core(mg_hierarchy* h, int lv, int precond, const double* dprec, DevBuf<double>& work, const double* b,
                double* x, long long inner, double tol, long long maxIter, long long* iters, long long* flag_out,
                double* resvec, long long* nres);
int block_fgmres_core(mg_hierarchy* h, int lv, int precond, const double* dprec, DevBuf<double>* work, const double* B,
                      double* X, long long inner, double tol, long long maxIter, long long* iters, long long* flag_out,
                      double* resvec, long long* nres);
// (mg_dd.inc) the Schwarz sweep as coarsest solve, enqueued on the stream being played; giving a borrowed handle back
int dd_coarse(mg_hierarchy* h, const double* b, double* x, bool x_zero);
void dd_detach(mg_hierarchy* h);
// x_zero: x holds zeros or need not be read (always so below a finer level, MGcycle.jl:63-64); only the Schwarz sweep reads x
int k_coarse(mg_hierarchy* h, int level, const double* b, double* x, bool x_zero = true) {
  const long long n = h->n_coarse;
  if (h->coarse_dd) {   // solveDDSerial(AT, b, x, LU, 1) (MGcycle.jl:140-143)
    ProfScope ps(h, level, MG_K_COARSE, 0.0);
    return dd_coarse(h, b, x, x_zero);
  }
  if (h->coarse_gmres) {
    // coarseSolveType "GMRES" (MGcycle.jl:152-168): x = 0; one restart of FGMRES(10), tol 0.01, M = d .* v with
    // d = relaxParam ./ diag(A_c) (defineCoarsestAinv, MGsetup.jl:334)
    ProfScope ps(h, level, MG_K_COARSE, 0.0);
    MG_TRY(k_fill(h, x, n * h->play->nrhs, 0.0));
    if (h->play->nrhs != 1)   // MGcycle.jl:166: KrylovMethods.blockFGMRES(Afun, b, 10, tol = 0.01, maxIter = 1, M = M2, X = x)
      return block_fgmres_core(h, level, 1, h->coarse_d.p, &h->kwc_blk, b, x, 10, 0.01, 1, nullptr, nullptr, nullptr, nullptr);
    return fgmres_core(h, level, 1, h->coarse_d.p, h->kwc, b, x, 10, 0.01, 1, nullptr, nullptr, nullptr, nullptr);
  }
  if (h->coarse_lu) {
    ProfScope ps(h, level, MG_K_COARSE, 12.0 * (double)(h->luLval.n + h->luUval.n) + 16.0 * (double)n * (double)h->play->nrhs);
    mgk::LuDev F;
    F.n = (int)n;
    F.Lptr = h->luLptr.p; F.Lcol = h->luLcol.p; F.Lval = h->luLval.p;
    F.Uptr = h->luUptr.p; F.Ucol = h->luUcol.p; F.Uval = h->luUval.p;
    F.p = h->luP.p; F.q = h->luQ.p;
    F.Lorder = h->luLorder.p; F.Llvl = h->luLlvl.p; F.nLlvl = h->nLlvl;
    F.Uorder = h->luUorder.p; F.Ulvl = h->luUlvl.p; F.nUlvl = h->nUlvl;
    if (!h->lu_multi) {
      hipLaunchKernelGGL(mgk::sptrsv_lu<double>, dim3(1), dim3(1024), 0, h->play->stream, F, b, x, h->luWork.p, (int)h->play->nrhs);
      HIP_TRY(hipGetLastError());
      return MG_OK;
    }
    const int nr = (int)h->play->nrhs;
    double* y = h->luWork.p;
    auto wave_blocks = [](long long waves) { return dim3((unsigned)((waves * 64 + mgk::BLK - 1) / mgk::BLK)); };
    // y = L \ b[p]: the levels ahead of the trailing block one launch each, the block through its inverse
    const int nLl = (int)h->luLlvl_h.size() - 1, nUl = (int)h->luUlvl_h.size() - 1;
    for (int l = 0; l < nLl; ++l) {
      const int t0 = h->luLlvl_h[(size_t)l], t1 = h->luLlvl_h[(size_t)l + 1];
      hipLaunchKernelGGL(mgk::sptrsv_level<true>, wave_blocks(t1 - t0), dim3(mgk::BLK), 0, h->play->stream, F,
                         reinterpret_cast<const int4*>(h->luLslot.p), t0, t1, b, y, nr);
    }
    if (h->luML > 0) {
      const int n0 = (int)n - h->luML;
      hipLaunchKernelGGL(mgk::sptrsv_tail_rhs, wave_blocks(h->luML), dim3(mgk::BLK), 0, h->play->stream, F, n0, b, y, h->luTail.p, nr);
      hipLaunchKernelGGL(mgk::tri_apply<true>, wave_blocks((long long)h->luML * nr), dim3(mgk::BLK), 0, h->play->stream,
                         h->luInvL.p, (h->luML + 63) / 64 * 64, h->luTail.p, y + (size_t)n0 * (size_t)nr, h->luML, nr);
    }
    // y = U \ y: the trailing block first, then the levels behind it
    if (h->luMU > 0) {
      const int n0 = (int)n - h->luMU;
      HIP_TRY(hipMemcpyAsync(h->luTail.p, y + (size_t)n0 * (size_t)nr, (size_t)h->luMU * (size_t)nr * sizeof(double),
                             hipMemcpyDeviceToDevice, h->play->stream));
      hipLaunchKernelGGL(mgk::tri_apply<false>, wave_blocks((long long)h->luMU * nr), dim3(mgk::BLK), 0, h->play->stream,
                         h->luInvU.p, (h->luMU + 63) / 64 * 64, h->luTail.p, y + (size_t)n0 * (size_t)nr, h->luMU, nr);
    }
    for (int l = 0; l < nUl; ++l) {
      const int t0 = h->luUlvl_h[(size_t)l], t1 = h->luUlvl_h[(size_t)l + 1];
      hipLaunchKernelGGL(mgk::sptrsv_level<false>, wave_blocks(t1 - t0), dim3(mgk::BLK), 0, h->play->stream, F,
                         reinterpret_cast<const int4*>(h->luUslot.p), t0, t1, b, y, nr);
    }
    hipLaunchKernelGGL(mgk::sptrsv_scatter, dim3((unsigned)((n * nr + mgk::BLK - 1) / mgk::BLK)), dim3(mgk::BLK), 0,
                       h->play->stream, h->luQ.p, y, x, (int)n, nr);
    HIP_TRY(hipGetLastError());
    return MG_OK;
  }
  ProfScope ps(h, level, MG_K_COARSE,
               8.0 * ((double)n * (double)n + 2.0 * (double)n * (double)h->play->nrhs));
  const long long waves = n * h->play->nrhs;
  const long long blocks = (waves * 64 + mgk::BLK - 1) / mgk::BLK;
  hipLaunchKernelGGL(mgk::dense_apply, dim3((unsigned)blocks), dim3(mgk::BLK), 0, h->play->stream,
                     h->Ainv.p, b, x, (int)n, (int)h->play->nrhs);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
// sum of squares of x[0..len) -> h->play->scalar (device); no sync
int k_sumsq(mg_hierarchy* h, const double* x, long long len) {
  ProfScope ps(h, 0, MG_K_NORM, 8.0 * (double)len);
  const int nb = std::min<long long>(h->nred_blocks, std::max<long long>(1, (len / 2 + mgk::BLK - 1) / mgk::BLK));
  hipLaunchKernelGGL(mgk::sumsq_partial, dim3(nb), dim3(mgk::BLK), 0, h->play->stream, x, len,
                     h->play->partial.p);
  launch_sum_final(h, h->play->partial.p, nb);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
// host value of sqrt(h->play->scalar); synchronises the stream
// h->play->scalar on the host (*h->h_scalar) once the stream has drained
int scalar_wait(mg_hierarchy* h) {
  if (!h->play->scalar_mirrored) HIP_TRY(hipMemcpyAsync(h->h_scalar, h->play->scalar.p, sizeof(double), hipMemcpyDeviceToHost, h->play->stream));
  h->play->scalar_mirrored = false;
  HIP_TRY(spin_sync(h->play->stream));
  return MG_OK;
}
int scalar_sync(mg_hierarchy* h, double* out) {
  MG_TRY(scalar_wait(h));
  *out = std::sqrt(*h->h_scalar);
  return MG_OK;
}
// host value of sqrt(sum of squares); synchronises the stream
int norm_sync(mg_hierarchy* h, const double* x, long long len, double* out) {
  MG_TRY(k_sumsq(h, x, len));
  return scalar_sync(h, out);
}

}  // namespace
