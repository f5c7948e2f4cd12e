// mg_complex.inc - part of libmgvcycle.so's single translation unit (included by mgvcycle.hip in this order; not compiled on its own).
// ComplexF64 / Int64 hierarchies (the _CF64 entry points of include/mgvcycle.h): generic CSR on one GPU, V / W / F / K cycles,
// pointwise, Jac-GMRES or Vanka relaxation (K and Jac-GMRES: CF64 handles and - option single_kcycle - CF32 ones, one right-hand side or - option kcycle_blocks - a block taken as one long vector; Vanka: both precisions, one right-hand side), dense-inverse, sparse-LU or GMRES coarsest solve
// (the last: one host synchronisation per solve; blocks of right-hand sides by its block form where the option coarse_gmres_blocks asks for it).  The state lives apart from the real levels (CxState);
// the handle's real side is never finalized, so every FP64 entry point refuses a CF64 handle.
// The ComplexF64 Krylov drivers on these hierarchies (mg_*_CFP64) follow in mg_complex_krylov.inc; their state is part of CxState.
// ComplexF32 / Int64 hierarchies (the _CF32 entry points; the reference's VAL = ComplexF32, singlePrecision) share all of it: the
// same CxState / CxLevel / CxMat with single values, and cx_upload, cx_spmv, cx_relax, cx_cycle, cx_finalize and the host forms of
// cycle / solve / spmv written once over the pair type (cx_t or cf_t).  Their coarsest solve stays ComplexF64 (widen bc, the CF64
// kernels, narrow xc), and the _CFP64 Krylov drivers take them with the single cycle as preconditioner (the mixed branch of
// getMultigridPreconditioner, SolveFuncs.jl:52-58).
// Blocks of right-hand sides (mg_block_*_CF64 here, mg_block_*_CFP64 in mg_complex_krylov.inc) take nrhs with each call: cx_spmv,
// cx_relax, cx_coarse and cx_cycle carry a column count nr (0: the single-vector path, untouched; >= 1: row-major blocks [n][nr] on
// the block work set of CxState, cx_block_ensure).  Everything a vector entry point and its block twin differ in - the checks, the
// buffers, the lengths, how a host array is staged - is answered by the selector CxCols, so each form between the C ABI and that
// core is written once: cx_cycle_host / cx_solve_host / cx_spmv_host (both precisions, vectors and blocks), cx_coarse_gmres_host,
// and in mg_complex_krylov.inc cx_krylov and cx_cycle_dev.
// adjointHierarchy on the resident hierarchy (mg_adjoint_hierarchy_CF64 / _CF32; cx_adjoint_hierarchy): every operator replaced by its
// conjugate transpose in HBM, for both precisions.
// Also here: the stand-alone factor applier behind mg_lu_*_CFP64 / _CFP32 / _FP32 (CxLuT<S>, written once over the stored value
// type; its extern "C" entry points sit beside the real applier's in mg_cabi.inc).
//
// Reference behaviour reproduced for VAL = ComplexF64:
//   recursiveCycle  src/Multigrid/MGcycle.jl:1-118, relax l.122-136, solveCoarsest l.177
//   solveMG         src/Multigrid/SolveFuncs.jl:3-39 (norm: sqrt(sum |r_i|^2))
//   SpMatMul        src/Multigrid/SpMatMul.jl:4-13: mul!(target, adjoint(AT), x, alpha, beta) - A = AT^H, conj'd at upload
typedef mgk::d2_t cx_t;
typedef mgk::f2_t cf_t;   // the pair type of a ComplexF32 (CF32) handle: the same state, cycle and kernels in single precision

// (the state types live beside mg_hierarchy, outside the anonymous namespace: the handle holds a CxState*)
// one operator of a CF64 hierarchy, generic CSR: complex values (A = AT^H) or real values (P, R)
// ---- stand-alone factor applier (mg_lu_*_CFP64 / _CFP32 / _FP32): state of its own, apart from the CF64 hierarchies ----
// Written once over the stored value type S of the kernels (mg_complex.hpp): cx_t (ComplexF64), cf_t (ComplexF32) or float.
// lu_store<S>: the host scalar the caller's values come in and how many of them make one value.
template <typename S> struct lu_store;
template <> struct lu_store<cx_t> { typedef double scalar; static constexpr int comps = 2; static constexpr int kind = 1; };
template <> struct lu_store<float> { typedef float scalar; static constexpr int comps = 1; static constexpr int kind = 2; };
template <> struct lu_store<cf_t> { typedef float scalar; static constexpr int comps = 2; static constexpr int kind = 3; };
// one resident set of factors: the plain ones (x[q] = U \ (L \ b[p])) or the conjugate-transposed ones of the adjoint solve
template <typename S>
struct CxLuSetT {
  DevBuf<int> Lptr, Lcol, Uptr, Ucol, P, Q, Lorder, Llvl, Uorder, Ulvl, Lslot, Uslot;
  DevBuf<S> Lval, Uval, invL, invU;
  int nLlvl = 0, nUlvl = 0;                // dependency levels of the whole factors (single-workgroup form)
  bool multi = false;                      // chip-wide form: per-level launches + dense trailing inverse
  int M = 0;                               // order of the trailing block held as an explicit inverse
  std::vector<int> Llvl_h, Ulvl_h;         // host copies of the level pointers ahead of / behind the trailing block
  ~CxLuSetT() {
    for (DevBuf<int>* d : {&Lptr, &Lcol, &Uptr, &Ucol, &P, &Q, &Lorder, &Llvl, &Uorder, &Ulvl, &Lslot, &Uslot}) d->release();
    for (DevBuf<S>* d : {&Lval, &Uval, &invL, &invU}) d->release();
  }
};
template <typename S>
struct CxLuT {
  int device = 0;
  long long n = 0;
  Options opt;
  hipStream_t stream = nullptr;
  std::vector<long long> Lptr, Lcol, Uptr, Ucol, p, q;   // the caller's factors (1-based): the adjoint set is derived from them
  std::vector<typename lu_store<S>::scalar> Lval, Uval;
  CxLuSetT<S>* fwd = nullptr;
  CxLuSetT<S>* adj = nullptr;
  DevBuf<S> work, tail, stage_b, stage_x, stage_t;
};
typedef CxLuSetT<cx_t> CxLuSet;
typedef CxLuT<cx_t> CxLu;

struct CxMat {
  bool set = false, cplx = false, wide = false;
  bool single = false;          // values in valf (a CF32 handle's operators); val otherwise
  long long n_rows = 0, n_cols = 0, nnz = 0;
  int nblocks = 0;
  long long max_row = 0;        // the longest row (sizes the accumulator of cx_rap_numeric)
  bool rows_sorted = true;      // every row's stored columns ascend (cx_upload): what cx_rap_numeric needs of a coarse operator's pattern
  DevBuf<int> rowptr, colidx, blk_row;
  DevBuf<long long> rowptr64;   // wide: >= 2^31 - 4096 non-zeros (or the option force_rowptr64)
  DevBuf<double> val;           // nnz real values, or 2*nnz interleaved (re, im)
  DevBuf<float> valf;           // the same in single
  const void* vals() const { return single ? static_cast<const void*>(valf.p) : static_cast<const void*>(val.p); }
  bool has_t = false;           // the transposed pattern of cx_colsumsq (built on the first SPAI re-setup of the level)
  DevBuf<int> t_ptr, t_perm;
  void release() {
    rowptr.release(); colidx.release(); blk_row.release(); rowptr64.release(); val.release(); valf.release();
    t_ptr.release(); t_perm.release();
    set = false;
    has_t = false;
  }
};

struct CxLevel {
  CxMat A, P, R;
  // (a CF32 handle keeps (re, im) float pairs in the same buffers: one double slot per complex value, see cx_len)
  DevBuf<double> d;            // relaxPrecs[l], complex
  bool relax_set = false;
  long long npre = 0, npost = 0, n = 0;
  DevBuf<double> b, r, x[2];   // complex scratch (CYCLEmem, MGdef.jl:56-60); x ping-pongs between the sweeps
  DevBuf<double> Bb, Br, Bx[2];   // the same for the block entry points (mg_block_*): row-major [n][blk_cap], see CxState::blk_cap
  // FGMRES_relaxation's Z and AZ (FGMRESmem, FGMRES.jl:1-30), column-major, allocated by mg_finalize only when the schedule needs them:
  DevBuf<double> relaxZ, relaxAZ;   // Jac-GMRES smoothing on this level: max(npre, npost) columns (memRelax)
  DevBuf<double> kZ, kAZ;           // the K-cycle's two FGMRES steps ON this level (levels 2 .. nl-1): 2 columns (memKcycle of the level above)
  // The same directions for a block of right-hand sides taken as one long vector (option kcycle_blocks): direction j is a row-major
  // block [n][blk_cap] at j * n * nr.  Part of the block work set (cx_block_ensure), allocated only where the schedule needs them.
  DevBuf<double> BrelaxZ, BrelaxAZ, BkZ, BkAZ;
  VankaCore* vanka = nullptr;       // relaxation type 2: the cells' blocks (mg_set_vanka_CF64 / _CF32), released with the handle
  int vanka_type = 0;
  void release_vanka() {
    if (vanka) { vanka->release(); delete vanka; vanka = nullptr; }
  }
};

struct CxState {
  std::vector<CxLevel> lev;
  bool finalized = false;
  bool single = false;         // a CF32 handle (mg_create_CF32): operators, relaxPrecs and level vectors in single; the coarsest solve,
                               // the Krylov operator K and every Krylov vector stay ComplexF64
  bool K_auto = false;         // K is As[1] widened (the system operator of a CF32 handle's drivers when none was set)
  DevBuf<double> cw_b, cw_x;   // CF32: the coarsest right-hand side widened, the coarsest solution before it is narrowed
  bool coarse_set = false, coarse_lu = false;
  CxLu* coarse_multi = nullptr;   // sparse factors of >= lu_multi_min_rows rows: the chip-wide form of the factor applier
  CxLuT<cf_t>* coarse_single = nullptr;   // CF32: ComplexF32 factors applied to the cycle's own bc (mg_set_coarse_lu_CF32_INT64), either form
  long long n_coarse = 0;
  DevBuf<double> Ainv;         // row-major n_c x n_c complex
  DevBuf<int> luLptr, luLcol, luUptr, luUcol, luP, luQ, luLorder, luLlvl, luUorder, luUlvl;
  DevBuf<double> luLval, luUval, luWork;
  int nLlvl = 0, nUlvl = 0;
  // coarseSolveType "GMRES" (mg_set_coarse_gmres_CF64; cx_coarse_gmres): the coarsest Jacobi vector d_c, the 11 basis vectors V and 10
  // preconditioned vectors Z (column-major, n_c apart), the scalar table with its pinned readback, two sets of partial sums (a pass reads
  // one and writes the other), and on a CF32 handle the coarsest operator widened to ComplexF64.  Sized by mg_finalize.
  bool coarse_gmres = false;
  DevBuf<double> cgD, cgV, cgZ, cgTab, cgPart;
  double* h_cgtab = nullptr;         // pinned
  CxMat cgA;
  // The same solve on a block of right-hand sides (option coarse_gmres_blocks; cx_coarse_block_gmres, kernels: mg_cxblk_coarse.hpp): 11
  // blocks V and 10 blocks Z (row-major [n_c][cb_cap]), two sets of k x k partials, the table of xi_0 and every H_ij with its pinned
  // readback, R1 of the Cholesky QR under way, and the solution Y of the block least squares on its way back.  Part of the block
  // work set: sized by cx_block_ensure for cb_cap columns, grown with nrhs, nothing allocated inside a cycle.
  int cb_cap = 0;
  DevBuf<double> cbV, cbZ, cbTab, cbPart, cbR1, cbY;
  double* h_cbtab = nullptr;         // pinned
  double* h_cbY = nullptr;           // pinned
  DevBuf<double> stage_b, partial;   // the fine right-hand side; per-row-block partials of ||r||^2
  // The FGMRES relaxation's own partials and scalars (Jac-GMRES smoothing, K-cycle; cx_fgmres_relax): it runs inside the Krylov drivers,
  // whose kpart / kscal must survive a cycle.  Scalar 0: ||r0||^2; step j: the 2 j + 3 scalars of its GRAM launch from 1 + j^2 + 2 j on,
  // so `inner` steps fill (inner + 1)^2 scalars; gpart holds one partial per scalar and row block (gpart[c * nblocks + block]).
  static constexpr int GSCAL = (mgk::GRAM_MAXV + 1) * (mgk::GRAM_MAXV + 1);
  DevBuf<double> gpart, gscal;
  double* h_gscal = nullptr;         // pinned
  // the Krylov drivers (mg_complex_krylov.inc): their system operator (unset: As[1]), work vectors, the partials and scalars of
  // the fused passes with the scalars' pinned readback, the iterate of the host-pointer forms
  static constexpr size_t KSCAL = 136;   // 2 * (64 + 2) doubles of an FGMRES(64) inner step, rounded up
  CxMat K;
  DevBuf<double> kwork, kpart, kscal, stage_x;
  double* h_kscal = nullptr;
  // The block work set of the mg_block_* entry points: sized lazily for blk_cap columns (cx_block_ensure), grown when a larger nrhs
  // arrives, dropped by mg_finalize.  The handle's own nrhs stays 1 and its single-vector state above is never touched by a block call.
  //   lev[l].Bb / Br / Bx[2]; the widened coarsest pair of a CF32 handle; the triangular sweeps' work vector; the staging blocks of the
  //   host forms (row-major b and x, and one column-major block); the Krylov blocks, Gram partials and coefficient slots of block BiCGSTAB
  int blk_cap = 0;
  DevBuf<double> Bcw_b, Bcw_x, BluWork, Bstage_b, Bstage_x, Bstage_t, Bkwork, Bgpart, Bcoef;
  double* h_bgram = nullptr;        // pinned: one k x k complex Gram matrix
  double* h_bcoef = nullptr;        // pinned ring of coefficient matrices
  unsigned bcoef_next = 0;
  std::vector<hipEvent_t> rap_ev;   // mg_rap_CF64: one event ahead of every level's kernels and one behind the last (mg_rap_level_ms_CF64)
  bool rap_timed = false;
  ~CxState() {
    for (hipEvent_t e : rap_ev) (void)hipEventDestroy(e);
    for (auto& L : lev) {
      L.A.release(); L.P.release(); L.R.release();
      L.d.release(); L.b.release(); L.r.release(); L.x[0].release(); L.x[1].release();
      L.Bb.release(); L.Br.release(); L.Bx[0].release(); L.Bx[1].release();
      L.relaxZ.release(); L.relaxAZ.release(); L.kZ.release(); L.kAZ.release();
      L.BrelaxZ.release(); L.BrelaxAZ.release(); L.BkZ.release(); L.BkAZ.release();
      L.release_vanka();
    }
    gpart.release(); gscal.release();
    if (h_gscal) (void)hipHostFree(h_gscal);
    for (DevBuf<double>* d : {&Bcw_b, &Bcw_x, &BluWork, &Bstage_b, &Bstage_x, &Bstage_t, &Bkwork, &Bgpart, &Bcoef}) d->release();
    if (h_bgram) (void)hipHostFree(h_bgram);
    if (h_bcoef) (void)hipHostFree(h_bcoef);
    Ainv.release();
    for (DevBuf<double>* d : {&cgD, &cgV, &cgZ, &cgTab, &cgPart}) d->release();
    if (h_cgtab) (void)hipHostFree(h_cgtab);
    cgA.release();
    for (DevBuf<double>* d : {&cbV, &cbZ, &cbTab, &cbPart, &cbR1, &cbY}) d->release();
    if (h_cbtab) (void)hipHostFree(h_cbtab);
    if (h_cbY) (void)hipHostFree(h_cbY);
    for (DevBuf<int>* d : {&luLptr, &luLcol, &luUptr, &luUcol, &luP, &luQ, &luLorder, &luLlvl, &luUorder, &luUlvl}) d->release();
    luLval.release(); luUval.release(); luWork.release();
    stage_b.release(); partial.release(); cw_b.release(); cw_x.release();
    K.release();
    kwork.release(); kpart.release(); kscal.release(); stage_x.release();
    if (h_kscal) (void)hipHostFree(h_kscal);
  }
};

namespace {

template <typename S> void cxlu_destroy(CxLuT<S>* S_);
// the factor appliers a hierarchy holds for its coarsest solve, released (another coarsest solve is being set, or the handle goes)
void cx_drop_coarse_appliers(CxState& S) {
  if (S.coarse_multi) { cxlu_destroy(S.coarse_multi); S.coarse_multi = nullptr; }
  if (S.coarse_single) { cxlu_destroy(S.coarse_single); S.coarse_single = nullptr; }
}
void cx_destroy(CxState* s) {
  cx_drop_coarse_appliers(*s);
  delete s;
}

template <typename C = cx_t>
inline C* cxp(DevBuf<double>& b) { return reinterpret_cast<C*>(b.p); }
template <typename C = cx_t>
inline const C* cxc(const DevBuf<double>& b) { return reinterpret_cast<const C*>(b.p); }
inline unsigned cx_grid(long long n) { return (unsigned)((n + mgk::BLK - 1) / mgk::BLK); }
template <typename T> struct cx_non_deduced { typedef T type; };   // (a nullptr argument must not take part in deducing C)
// doubles that hold n complex values of the handle's precision
inline size_t cx_len(const CxState& S, long long n) { return (S.single ? 1 : 2) * (size_t)n; }

// which handles an entry point serves: the _CF64 ones CF64 handles, the _CF32 ones CF32 handles, the coarsest-solve setters and
// the _CFP64 Krylov entry points both
enum CxWant { CX_WANT64, CX_WANT32, CX_ANY };
int cx_handle_ok(mg_hierarchy* h, CxWant want) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  if (!h->cx) return fail(MG_ERR_STATE, "complex entry point called on an FP64 handle (create it with mg_create_CF64 or mg_create_CF32)");
  if (want == CX_WANT64 && h->cx->single) return fail(MG_ERR_STATE, "CF64 entry point called on a CF32 handle (its _CF32 twin serves it)");
  if (want == CX_WANT32 && !h->cx->single) return fail(MG_ERR_STATE, "CF32 entry point called on a CF64 handle (create it with mg_create_CF32)");
  return MG_OK;
}
int cx_level_ok(mg_hierarchy* h, long long level, CxWant want = CX_WANT64) {
  MG_TRY(cx_handle_ok(h, want));
  if (level < 1 || level > h->nlevels) return fail(MG_ERR_INVALID, "bad level %lld", level);
  return MG_OK;
}
// what a CF32 handle does not serve (device re-setup, reading values back)
#define MG_CF32_UNSUPPORTED(h)                                                                                       \
  do {                                                                                                               \
    if ((h) && (h)->cx && (h)->cx->single) return fail(MG_ERR_UNSUPPORTED, "%s is not served for CF32 handles", __func__); \
  } while (0)

// Upload one operator from the reference's CSC-of-AT arrays (1-based Int64).  Complex values are conjugated here, once:
// the kernels then compute y_i = sum_k val_k x[col_k] = (AT^H x)_i.
template <typename ST>
int cx_upload(CxMat* M, const Options& opt, long long n_rows, long long n_cols, const long long* colptr, const long long* rowval,
              const ST* nzval, bool cplx) {
  constexpr bool single = sizeof(ST) == sizeof(float);
  if (n_rows < 1 || n_cols < 1 || !colptr || !rowval || !nzval) return fail(MG_ERR_INVALID, "empty operator or null array");
  if (n_rows >= (1LL << 31) - 1 || n_cols >= (1LL << 31) - 1) return fail(MG_ERR_UNSUPPORTED, "dimension exceeds int32 device indices");
  if (colptr[0] != 1) return fail(MG_ERR_INVALID, "colptr[1] must be 1 (1-based Julia arrays expected)");
  const long long nnz = colptr[n_rows] - 1;
  if (nnz < 0) return fail(MG_ERR_INVALID, "colptr is not a 1-based pointer array");
  std::vector<long long> rp((size_t)n_rows + 1);
  for (long long i = 0; i <= n_rows; ++i) {
    const long long v = colptr[i] - 1;
    if (v < 0 || v > nnz || (i > 0 && v < rp[(size_t)i - 1]))
      return fail(MG_ERR_INVALID, "colptr is not a monotone 1-based pointer array at %lld", i);
    rp[(size_t)i] = v;
  }
  std::vector<int> ci((size_t)std::max<long long>(nnz, 1), 0);
  for (long long k = 0; k < nnz; ++k) {
    const long long c = rowval[k] - 1;
    if (c < 0 || c >= n_cols) return fail(MG_ERR_INVALID, "rowval[%lld]=%lld outside 1..%lld", k + 1, rowval[k], n_cols);
    ci[(size_t)k] = (int)c;
  }
  // row blocks: consecutive rows, <= MAXROWS rows and <= CX_CHUNK non-zeros (a longer row has a block of its own)
  std::vector<int> blk(1, 0);
  for (long long r = 0; r < n_rows;) {
    long long e = r + 1;
    while (e < n_rows && (e - r) < mgk::MAXROWS && rp[(size_t)e + 1] - rp[(size_t)r] <= mgk::CX_CHUNK) ++e;
    blk.push_back((int)e);
    r = e;
  }
  const size_t vw = cplx ? 2 : 1;
  std::vector<ST> v((size_t)std::max<long long>(nnz, 1) * vw, ST(0));
  for (long long k = 0; k < (long long)nnz * (long long)vw; ++k) v[(size_t)k] = (cplx && (k & 1)) ? -nzval[k] : nzval[k];
  M->release();
  M->cplx = cplx;
  M->single = single;
  M->wide = nnz >= (1LL << 31) - 4096 || opt.force_rowptr64;
  M->n_rows = n_rows;
  M->n_cols = n_cols;
  M->nnz = nnz;
  M->nblocks = (int)blk.size() - 1;
  M->max_row = 0;
  M->rows_sorted = true;
  for (long long i = 0; i < n_rows; ++i) {
    M->max_row = std::max(M->max_row, rp[(size_t)i + 1] - rp[(size_t)i]);
    for (long long k = rp[(size_t)i] + 1; k < rp[(size_t)i + 1] && M->rows_sorted; ++k)
      if (ci[(size_t)k] < ci[(size_t)k - 1]) M->rows_sorted = false;
  }
  if (M->wide) {
    MG_TRY(M->rowptr64.alloc(rp.size()));
    HIP_TRY(hipMemcpy(M->rowptr64.p, rp.data(), rp.size() * sizeof(long long), hipMemcpyHostToDevice));
  } else {
    std::vector<int> rp32(rp.begin(), rp.end());
    MG_TRY(M->rowptr.alloc(rp32.size()));
    HIP_TRY(hipMemcpy(M->rowptr.p, rp32.data(), rp32.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  MG_TRY(M->colidx.alloc(ci.size()));
  if (single) MG_TRY(M->valf.alloc(v.size()));
  else MG_TRY(M->val.alloc(v.size()));
  MG_TRY(M->blk_row.alloc(blk.size()));
  HIP_TRY(hipMemcpy(M->colidx.p, ci.data(), ci.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(const_cast<void*>(M->vals()), v.data(), v.size() * sizeof(ST), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(M->blk_row.p, blk.data(), blk.size() * sizeof(int), hipMemcpyHostToDevice));
  M->set = true;
  return MG_OK;
}

// P or R of a CF64 handle (mg_set_operator_FP64_INT64 routes them here): real values, applied to complex vectors
int cx_set_transfer(mg_hierarchy* h, long long level, long long which, long long n_rows, long long n_cols, const long long* colptr,
                    const long long* rowval, const double* nzval) {
  if (h && h->cx && h->cx->single)
    return fail(MG_ERR_STATE, "mg_set_operator_FP64_INT64 on a CF32 handle: Ps and Rs are Float32 (mg_set_operator_CF32_INT64)");
  MG_TRY(cx_level_ok(h, level));
  if (which == MG_OP_A)
    return fail(MG_ERR_STATE, "mg_set_operator_FP64_INT64(MG_OP_A) on a CF64 handle: As are complex (mg_set_operator_CF64_INT64)");
  if (which != MG_OP_P && which != MG_OP_R) return fail(MG_ERR_INVALID, "bad operator selector %lld", which);
  if (level == h->nlevels) return fail(MG_ERR_INVALID, "the coarsest level %lld has no transfer operators", level);
  (void)hipSetDevice(h->device);
  CxLevel& L = h->cx->lev[(size_t)level - 1];
  MG_TRY(cx_upload(which == MG_OP_P ? &L.P : &L.R, h->opt, n_rows, n_cols, colptr, rowval, nzval, false));
  h->cx->finalized = false;
  return MG_OK;
}

// y = epilogue(M * x) on h's stream; the launch of one (MODE, row-pointer width, value type, pair type).  nr == 0: vectors, the
// one-lane-per-row kernel; nr >= 1: row-major blocks [n][nr], the block kernel on the same row blocks (G = pow2 >= nr lanes per row)
template <int MODE, typename PTR, typename VT, typename C>
void cx_launch(mg_hierarchy* h, const CxMat& M, const PTR* rowptr, const mgk::CxVecArgsT<C>& v, int nr) {
  mgk::CxCsrDev<PTR, VT> D;
  D.rowptr = rowptr;
  D.colidx = M.colidx.p;
  D.val = static_cast<const VT*>(M.vals());
  D.blk_row = M.blk_row.p;
  D.nblocks = M.nblocks;
  D.n_rows = (int)M.n_rows;
  if (nr == 0) {
    hipLaunchKernelGGL((mgk::cx_csr_stream_spmv<MODE, PTR, VT, C>), dim3((unsigned)M.nblocks), dim3(mgk::BLK), 0, h->play->stream, D, v);
    return;
  }
  int lg = 0;
  while ((1 << lg) < nr) ++lg;
  hipLaunchKernelGGL((mgk::cx_csr_stream_spmm<MODE, PTR, VT, C>), dim3((unsigned)M.nblocks), dim3(mgk::BLK), 0, h->play->stream, D, v, nr, lg);
}

// C: the pair type of the vectors (cx_t or cf_t), deduced from x; the operator holds values of the same precision; nr as for cx_launch
template <int MODE, typename C>
int cx_spmv(mg_hierarchy* h, const CxMat& M, const C* x, typename cx_non_deduced<C>::type* y, const typename cx_non_deduced<C>::type* b,
            const typename cx_non_deduced<C>::type* d, double* sumsq, typename cx_non_deduced<C>::type alpha = C{1, 0},
            typename cx_non_deduced<C>::type beta = C{0, 0}, int nr = 0, typename cx_non_deduced<C>::type* z1 = nullptr) {
  typedef typename mgk::cx_scalar<C>::type T;
  if (M.single != (sizeof(T) == sizeof(float))) return fail(MG_ERR_INVALID, "internal: operator and vectors differ in precision");
  if (nr < 0 || nr > mgk::BLK_KMAX) return fail(MG_ERR_INVALID, "internal: a block of %d columns", nr);
  mgk::CxVecArgsT<C> v = {};
  v.x = x; v.y = y; v.b = b; v.d = d; v.sumsq = sumsq;
  v.alpha = alpha; v.beta = beta;
  v.beta_zero = (beta.x == 0 && beta.y == 0) ? 1 : 0;
  if (z1 && (MODE != mgk::RESID || !d)) return fail(MG_ERR_INVALID, "internal: z1 = d.*r comes out of the residual only");
  v.z1 = z1;
  if (M.cplx) {
    if (M.wide) cx_launch<MODE, long long, C, C>(h, M, M.rowptr64.p, v, nr);
    else cx_launch<MODE, int, C, C>(h, M, M.rowptr.p, v, nr);
  } else {
    if (MODE != mgk::AXPBY) return fail(MG_ERR_INVALID, "internal: a real transfer operator serves the AXPBY form only");
    if (M.wide) cx_launch<mgk::AXPBY, long long, T, C>(h, M, M.rowptr64.p, v, nr);
    else cx_launch<mgk::AXPBY, int, T, C>(h, M, M.rowptr.p, v, nr);
  }
  HIP_TRY(hipGetLastError());
  return MG_OK;
}

// ||z||^2 = sum |z_i|^2 into the pinned host scalar: the two-pass deterministic sum
template <typename C>
int cx_norm2(mg_hierarchy* h, const C* z, long long n, double* out) {
  const int np = (int)std::min<long long>(h->nred_blocks, std::max<long long>(1, (n + mgk::BLK - 1) / mgk::BLK));
  hipLaunchKernelGGL(mgk::cx_sumsq_partial<C>, dim3((unsigned)np), dim3(mgk::BLK), 0, h->play->stream, z, n, h->play->partial.p);
  hipLaunchKernelGGL(mgk::sum_final, dim3(1), dim3(mgk::BLK), 0, h->play->stream, h->play->partial.p, np, h->play->scalar.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h->h_scalar, h->play->scalar.p, sizeof(double), hipMemcpyDeviceToHost, h->play->stream));
  HIP_TRY(spin_sync(h->play->stream));
  *out = h->h_scalar[0];
  return MG_OK;
}

// r = b - A x with the per-block partials of ||r||^2, then the sum into the pinned host scalar
// (nr >= 1: blocks [n][nr], the sum over all columns - the Frobenius norm of the block solveMG)
template <typename C>
int cx_residual_norm2(mg_hierarchy* h, const CxLevel& L, const C* b, const C* x, C* r, double* out, int nr = 0) {
  CxState& S = *h->cx;
  MG_TRY(cx_spmv<mgk::RESID>(h, L.A, x, r, b, nullptr, S.partial.p, C{1, 0}, C{0, 0}, nr));
  hipLaunchKernelGGL(mgk::sum_final, dim3(1), dim3(mgk::BLK), 0, h->play->stream, S.partial.p, L.A.nblocks, h->play->scalar.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h->h_scalar, h->play->scalar.p, sizeof(double), hipMemcpyDeviceToHost, h->play->stream));
  HIP_TRY(spin_sync(h->play->stream));
  *out = h->h_scalar[0];
  return MG_OK;
}

// the two conversion passes (mgk::cx_narrow / cx_widen) on h's stream
int cx_narrow(mg_hierarchy* h, const cx_t* src, cf_t* dst, long long n) {
  hipLaunchKernelGGL(mgk::cx_narrow, dim3(cx_grid(n)), dim3(mgk::BLK), 0, h->play->stream, src, dst, n);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
int cx_widen(mg_hierarchy* h, const cf_t* src, cx_t* dst, long long n) {
  hipLaunchKernelGGL(mgk::cx_widen, dim3(cx_grid(n)), dim3(mgk::BLK), 0, h->play->stream, src, dst, n);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}

template <typename S>
int cxlu_solve_dev(CxLuT<S>* S_, CxLuSetT<S>& G, const S* b, S* x, int nr, const hipStream_t* on = nullptr);

// ---- coarseSolveType "GMRES" (MGsetup.jl:335-336, MGcycle.jl:152-164) for complex hierarchies -------------------------------------------
// x .= 0, then ONE restart of KrylovMethods.fgmres(A_c, b, 10, tol = 0.01, maxIter = 1, M = v -> d_c .* v).  The restart is enqueued
// speculatively and whole, as cx_fgmres_relax enqueues a relaxation: the front, all 10 Arnoldi steps (kernels and table: mg_cxvec.hpp),
// ONE readback of the 121 scalars, ONE host synchronisation; the host then replays the columns (coarse_gmres_replay,
// mg_krylov_host.hpp), which fixes `used`, and x = Z[:, :used] y is one more pass.  Columns behind the break were computed and are not
// read.  b = 0: x = 0 and flag -9, as the reference returns.  (The reference's fgmres also looks at the true residual behind a restart
// that did not meet tol; in exact arithmetic that residual is the last estimate, and nothing in the cycle reads the flag.)
constexpr double CX_CG_TOL = 0.01;
// levels of at most this many rows take the one-workgroup tail (cg_tail) behind every product, larger ones the chain of passes
// (measured: profiles/complex_coarse_gmres.md); the option coarse_gmres_tail_rows moves the threshold (0: the chain everywhere)
constexpr long long CX_CG_TAIL_DEFAULT_ROWS = mgcv::CG_TAIL_ROWS;
static_assert(mgcv::CG_TAIL_ROWS >= 4913, "the one-workgroup tail serves every geometric coarsest level up to 17^3 rows");

inline bool cx_cg_use_tail(const mg_hierarchy* h) {
  const long long opt = h->opt.coarse_gmres_tail_rows;
  const long long lim = std::min<long long>(opt < 0 ? CX_CG_TAIL_DEFAULT_ROWS : opt, mgcv::CG_TAIL_ROWS);
  return h->cx->n_coarse <= lim;
}
// kernel launches of one solve on the path in use: the front, the 10 steps, the combination (b = 0 skips the last)
inline long long cx_cg_launches(const mg_hierarchy* h) {
  if (cx_cg_use_tail(h)) return 1 + 2 * mgcv::CG_M + 1;
  long long c = 2 + 1;
  for (int i = 0; i < mgcv::CG_M; ++i) c += i + 3;
  return c;
}
// the coarsest operator the solve applies: the level's own on a CF64 handle, its widened copy on a CF32 one
inline const CxMat& cx_cg_operator(const CxState& S) { return S.single ? S.cgA : S.lev.back().A; }

// w = A z with the partials of dot(v0, w) at part (re: [0, nblocks), im: [nblocks, 2 nblocks))
int cx_cg_product(mg_hierarchy* h, const CxMat& M, const cx_t* z, cx_t* w, const cx_t* v0, double* part) {
  mgk::CxVecArgsT<cx_t> v = {};
  v.x = z;
  v.y = w;
  v.beta_zero = 1;
  v.r0 = v0;
  v.gpart = part;
  if (M.wide) {
    mgk::CxCsrDev<long long, cx_t> D;
    D.rowptr = M.rowptr64.p; D.colidx = M.colidx.p; D.val = static_cast<const cx_t*>(M.vals()); D.blk_row = M.blk_row.p;
    D.nblocks = M.nblocks; D.n_rows = (int)M.n_rows;
    hipLaunchKernelGGL((mgk::cx_csr_stream_spmv<mgk::CGDOT, long long, cx_t, cx_t>), dim3((unsigned)M.nblocks), dim3(mgk::BLK), 0, h->play->stream, D, v);
  } else {
    mgk::CxCsrDev<int, cx_t> D;
    D.rowptr = M.rowptr.p; D.colidx = M.colidx.p; D.val = static_cast<const cx_t*>(M.vals()); D.blk_row = M.blk_row.p;
    D.nblocks = M.nblocks; D.n_rows = (int)M.n_rows;
    hipLaunchKernelGGL((mgk::cx_csr_stream_spmv<mgk::CGDOT, int, cx_t, cx_t>), dim3((unsigned)M.nblocks), dim3(mgk::BLK), 0, h->play->stream, D, v);
  }
  HIP_TRY(hipGetLastError());
  return MG_OK;
}

// what a caller may ask back of one coarsest solve (mg_coarse_gmres_CF64)
struct CxCoarseReport {
  int used = 0;
  long long flag = 0;
  double resvec[mgcv::CG_M] = {};
};

int cx_coarse_gmres(mg_hierarchy* h, const cx_t* b, cx_t* x, CxCoarseReport* report = nullptr) {
  CxState& S = *h->cx;
  const CxMat& A = cx_cg_operator(S);
  const long long n = S.n_coarse;
  const size_t ld = (size_t)n;
  const hipStream_t st = h->play->stream;
  constexpr int m = mgcv::CG_M;
  if (!A.set || S.cgV.n != 2 * ld * (m + 1) || !S.h_cgtab) return fail(MG_ERR_STATE, "internal: the GMRES coarsest solve's work set is not sized");
  cx_t *V = cxp(S.cgV), *Z = cxp(S.cgZ);
  const cx_t* d = cxc(S.cgD);
  double* tab = S.cgTab.p;
  const size_t P = S.cgPart.n / 4;
  double* part[2] = {S.cgPart.p, S.cgPart.p + 2 * P};
  const bool tail = cx_cg_use_tail(h);
  const int G = mgcv::cxv_grid(n);
  const unsigned T = (unsigned)std::min<long long>(mgcv::CG_TAIL_T, (n + 63) / 64 * 64);
  // front: r = b (x = 0); ||b||^2, v_0 = b / ||b||, z_0 = d.*v_0
  if (tail) {
    hipLaunchKernelGGL(mgcv::cg_tail, dim3(1), dim3(T), 0, st, (const double*)nullptr, 0, 0, tab, (const cx_t*)V, (long long)ld, b, V, d, Z, (int)n);
  } else {
    hipLaunchKernelGGL(mgk::cx_sumsq_partial<cx_t>, dim3((unsigned)G), dim3(mgk::BLK), 0, st, b, n, part[0]);
    hipLaunchKernelGGL(mgcv::cg_norm_pass, dim3((unsigned)G), dim3(mgcv::KB), 0, st, (const double*)part[0], G, tab, b, V, d, Z, n);
  }
  HIP_TRY(hipGetLastError());
  for (int i = 0; i < m; ++i) {
    cx_t* w = V + (size_t)(i + 1) * ld;
    cx_t* znext = i + 1 < m ? Z + (size_t)(i + 1) * ld : nullptr;
    double* slot = tab + mgcv::cg_slot(i);
    MG_TRY(cx_cg_product(h, A, Z + (size_t)i * ld, w, V, part[0]));
    if (tail) {
      hipLaunchKernelGGL(mgcv::cg_tail, dim3(1), dim3(T), 0, st, (const double*)part[0], A.nblocks, i + 1, slot, (const cx_t*)V, (long long)ld,
                         (const cx_t*)w, w, d, znext, (int)n);
    } else {
      int cur = 0, np = A.nblocks;
      for (int k = 0; k <= i; ++k) {
        hipLaunchKernelGGL(mgcv::cg_mgs_pass, dim3((unsigned)G), dim3(mgcv::KB), 0, st, (const double*)part[cur], np, slot + 2 * k,
                           (const cx_t*)(V + (size_t)k * ld), k < i ? (const cx_t*)(V + (size_t)(k + 1) * ld) : (const cx_t*)nullptr, w, n, part[1 - cur]);
        cur = 1 - cur;
        np = G;
      }
      hipLaunchKernelGGL(mgcv::cg_norm_pass, dim3((unsigned)G), dim3(mgcv::KB), 0, st, (const double*)part[cur], np, slot + 2 * (i + 1), (const cx_t*)w, w, d,
                         znext, n);
    }
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(S.h_cgtab, tab, sizeof(double) * mgcv::CG_TAB, hipMemcpyDeviceToHost, st));
  HIP_TRY(spin_sync(st));
  HessenbergLsq<std::complex<double>> Q(m);
  CxCoarseReport local;
  CxCoarseReport& R = report ? *report : local;
  coarse_gmres_replay(S.h_cgtab, CX_CG_TOL, Q, R.used, R.flag, R.resvec);
  if (R.used == 0) {   // b = 0
    HIP_TRY(hipMemsetAsync(x, 0, sizeof(cx_t) * ld, st));
    return MG_OK;
  }
  mgcv::OpCCombine op;
  op.m = R.used;
  op.x = x;
  for (int j = 0; j < m; ++j) {
    const int jj = j < R.used ? j : 0;
    op.y[j] = j < R.used ? cx_t{Q.y[(size_t)j].real(), Q.y[(size_t)j].imag()} : cx_t{0.0, 0.0};
    op.z[j] = Z + (size_t)jj * ld;
  }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(mgcv::cxv_pass<mgcv::OpCCombine>), dim3((unsigned)G), dim3(mgcv::KB), 0, st, op, n, part[0]);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}

// ---- the same for a block of right-hand sides (MGcycle.jl:165-167; option coarse_gmres_blocks) ------------------------------------------
// X .= 0, then ONE restart of KrylovMethods.blockFGMRES(A_c, B, 10, tol = 0.01, maxIter = 1, M = V -> d_c .* V) on row-major blocks
// [n_c][k], 2 <= k <= BLK_KMAX.  Enqueued speculatively and whole, as cx_coarse_gmres does it for a vector (kernels: mg_cxblk_coarse.hpp):
//   front    B^H B (cx_blk_gram_onepass), the two passes of cholqr2(B): V_0, xi_0, ||B||_F^2, Z_0 = d.*V_0           3 launches
//   step j   W = A_c Z_j (cx_csr_stream_spmm), V_0^H W (cx_blk_gram_onepass), j + 1 Gram-Schmidt passes, the two
//            passes of cholqr2(W) with Z_{j+1} = d.*V_{j+1}                                                              j + 5 launches
// then ONE copy of the table (||B||_F^2, xi_0, every H_ij and H_{j+1,j}) and ONE host synchronisation; the host replays the block
// least squares (coarse_block_gmres_replay, mg_krylov_host.hpp), which fixes `used`, and X = sum_{j < used} Z_j Y_j is the copy of Y
// and one more launch.  B = 0: X = 0 and flag -9.  The columns of a block are coupled: this is NOT k single-vector solves.
// The first Gram matrix of a step is a launch of the existing one-pass kernel, not an epilogue of the product (see
// profiles/complex_block_coarse_gmres.md).  Blocks of few values take the one-workgroup form of everything behind the product instead
// (cb_tail: 1 launch for the front, 2 per step; cx_cb_use_tail).
inline int cb_lg(int k) {
  int l = 0;
  while ((1 << l) < k) ++l;
  return l;
}
// Blocks of at most this many values (n_c * k) take the one-workgroup form (cb_tail) behind every product, larger ones the chain of
// passes (measured: profiles/complex_block_coarse_gmres.md).  The option coarse_gmres_tail_rows moves the threshold for blocks too: it
// is then compared with n_c * k (0: the chain everywhere; capped by the form's limit).
constexpr long long CX_CB_TAIL_DEFAULT_ENTRIES = 1024;   // (a single tile at every k: it lost at 125 x 16 = 2000 values, two tiles)
inline bool cx_cb_use_tail(const mg_hierarchy* h, int k) {
  const long long opt = h->opt.coarse_gmres_tail_rows;
  const long long lim = std::min<long long>(opt < 0 ? CX_CB_TAIL_DEFAULT_ENTRIES : opt, mgcb::CB_TAIL_ENTRIES);
  return h->cx->n_coarse * k <= lim;
}
// kernel launches of one block solve of k columns on the path in use: the front, the 10 steps, the combination (B = 0 skips the last)
inline long long cx_cb_launches(const mg_hierarchy* h, int k) {
  if (cx_cb_use_tail(h, k)) return 1 + 2 * mgcb::CB_M + 1;
  long long c = 3 + 1;
  for (int j = 0; j < mgcb::CB_M; ++j) c += j + 5;
  return c;
}
int cx_cb_ensure(mg_hierarchy* h, int nr) {
  CxState& S = *h->cx;
  if (!S.coarse_gmres || !h->opt.coarse_gmres_blocks || nr <= 1 || nr <= S.cb_cap) return MG_OK;
  (void)hipSetDevice(h->device);
  HIP_TRY(spin_sync(h->play->stream));   // (an earlier block call may still read the buffers replaced below)
  S.cb_cap = 0;
  constexpr int m = mgcb::CB_M;
  const size_t len = 2 * (size_t)S.n_coarse * (size_t)nr, kk = 2 * (size_t)nr * nr;
  const size_t tlen = coarse_block_table_len(nr, m);
  MG_TRY(S.cbV.alloc(len * (m + 1)));
  MG_TRY(S.cbZ.alloc(len * m));
  MG_TRY(S.cbTab.alloc(tlen));
  MG_TRY(S.cbPart.alloc(2 * (size_t)mgcb::CB_MAXWG * kk));
  MG_TRY(S.cbR1.alloc(kk));
  MG_TRY(S.cbY.alloc(kk * m));
  if (S.h_cbtab) (void)hipHostFree(S.h_cbtab);
  if (S.h_cbY) (void)hipHostFree(S.h_cbY);
  S.h_cbtab = S.h_cbY = nullptr;
  HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&S.h_cbtab), sizeof(double) * tlen));
  HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&S.h_cbY), sizeof(double) * kk * m));
  S.cb_cap = nr;
  return MG_OK;
}

int cx_coarse_block_gmres(mg_hierarchy* h, const cx_t* b, cx_t* x, int k, CxCoarseReport* report = nullptr) {
  CxState& S = *h->cx;
  const CxMat& A = cx_cg_operator(S);
  const long long n = S.n_coarse;
  const size_t len = (size_t)n * (size_t)k, kk = (size_t)k * k;
  const hipStream_t st = h->play->stream;
  constexpr int m = mgcb::CB_M;
  if (k < 2 || k > mgk::BLK_KMAX) return fail(MG_ERR_INVALID, "internal: a block GMRES coarsest solve of %d columns", k);
  if (!A.set || S.cb_cap < k || !S.h_cbtab || S.cgD.n != 2 * (size_t)n) return fail(MG_ERR_STATE, "internal: the block GMRES coarsest solve's work set is not sized");
  cx_t *V = cxp(S.cbV), *Z = cxp(S.cbZ);
  const cx_t* d = cxc(S.cgD);
  cx_t* tab = cxp(S.cbTab) + 1;                      // (entry 0 of the table: ||B||_F^2 and a pad)
  cx_t* part[2] = {cxp(S.cbPart), cxp(S.cbPart) + (size_t)mgcb::CB_MAXWG * kk};
  const int lg = cb_lg(k), G = mgcb::cb_grid(n, lg);
  const dim3 grid((unsigned)G), blk(mgk::BLK);
  mgcb::CbPass p = {};
  p.np = G; p.k = k; p.lgk = lg; p.n = n; p.d = d;
  auto chol2 = [&](const cx_t* src, cx_t* W, int cur, cx_t* out, double* trace, cx_t* znext) {   // cholqr2(src) -> W; the Gram partials at part[cur]
    mgcb::CbPass c = p;
    c.pprev = part[cur]; c.src = src; c.W = W; c.out = cxp(S.cbR1); c.trace = trace; c.pout = part[1 - cur];
    hipLaunchKernelGGL(mgcb::cb_pass<mgcb::CB_CHOL>, grid, blk, 0, st, c);
    c.pprev = part[1 - cur]; c.src = W; c.out = out; c.r1 = cxc(S.cbR1); c.trace = nullptr; c.pout = nullptr; c.Z = znext;
    hipLaunchKernelGGL(mgcb::cb_pass<mgcb::CB_CHOL>, grid, blk, 0, st, c);
  };
  const bool tail = cx_cb_use_tail(h, k);
  mgcb::CbTail t = {};
  t.k = k; t.lgk = lg; t.n = n; t.ld = (long long)len; t.V = V; t.d = d; t.r1 = cxp(S.cbR1); t.part = part[0];
  // front: R = B (X = 0); V_0, xi_0 = cholqr2(B), Z_0 = d.*V_0
  if (tail) {
    mgcb::CbTail f = t;
    f.nk = 0; f.src = b; f.W = V; f.Z = Z; f.slot = tab; f.trace = S.cbTab.p;
    hipLaunchKernelGGL(mgcb::cb_tail, dim3(1), blk, 0, st, f);
  } else {
    hipLaunchKernelGGL(mgk::cx_blk_gram_onepass, grid, blk, 0, st, b, b, n, k, lg, part[0]);
    chol2(b, V, 0, tab, S.cbTab.p, Z);
  }
  HIP_TRY(hipGetLastError());
  for (int j = 0; j < m; ++j) {
    cx_t* W = V + (size_t)(j + 1) * len;
    cx_t* slot = tab + coarse_block_slot(j) * kk;
    MG_TRY(cx_spmv<mgk::AXPBY>(h, A, Z + (size_t)j * len, W, nullptr, nullptr, nullptr, cx_t{1, 0}, cx_t{0, 0}, k));   // W = A_c Z_j
    if (tail) {
      mgcb::CbTail f = t;
      f.nk = j + 1; f.src = W; f.W = W; f.Z = j + 1 < m ? Z + (size_t)(j + 1) * len : nullptr; f.slot = slot;
      hipLaunchKernelGGL(mgcb::cb_tail, dim3(1), blk, 0, st, f);
      HIP_TRY(hipGetLastError());
      continue;
    }
    hipLaunchKernelGGL(mgk::cx_blk_gram_onepass, grid, blk, 0, st, (const cx_t*)V, (const cx_t*)W, n, k, lg, part[0]);   // V_0^H W
    int cur = 0;
    for (int i = 0; i <= j; ++i) {   // W -= V_i H_ij ; the partials of V_{i+1}^H W, at the end of W^H W
      mgcb::CbPass c = p;
      c.pprev = part[cur]; c.W = W; c.V = V + (size_t)i * len; c.U = i < j ? V + (size_t)(i + 1) * len : nullptr;
      c.out = slot + (size_t)i * kk; c.pout = part[1 - cur];
      hipLaunchKernelGGL(mgcb::cb_pass<mgcb::CB_MGS>, grid, blk, 0, st, c);
      cur = 1 - cur;
    }
    chol2(W, W, cur, slot + (size_t)(j + 1) * kk, nullptr, j + 1 < m ? Z + (size_t)(j + 1) * len : nullptr);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(S.h_cbtab, S.cbTab.p, sizeof(double) * coarse_block_table_len(k, m), hipMemcpyDeviceToHost, st));
  HIP_TRY(spin_sync(st));
  BlockHessenbergLsq Q(k, m);
  SmallMatC Y;
  CxCoarseReport local;
  CxCoarseReport& R = report ? *report : local;
  coarse_block_gmres_replay(S.h_cbtab, k, CX_CG_TOL, Q, R.used, R.flag, R.resvec, Y);
  if (R.used == 0) {   // B = 0
    HIP_TRY(hipMemsetAsync(x, 0, sizeof(cx_t) * len, st));
    return MG_OK;
  }
  const size_t ny = (size_t)R.used * kk;
  for (size_t e = 0; e < ny; ++e) {
    S.h_cbY[2 * e] = Y.a[e].real();
    S.h_cbY[2 * e + 1] = Y.a[e].imag();
  }
  HIP_TRY(hipMemcpyAsync(S.cbY.p, S.h_cbY, sizeof(cx_t) * ny, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(mgcb::cb_combine, dim3(std::min(cx_grid((long long)len), 4096u)), blk, 0, st, (const cx_t*)Z, (long long)len, R.used, cxc(S.cbY), x, n, k);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}

// ---- the work set of a call: everything a vector entry point and its block twin differ in -------------------------------------------
// nr == 0: one right-hand side on the handle's own buffers (the one-lane-per-row kernels); nr >= 1: a row-major block [n][nr] on the
// block work set (the block kernels, also for nr == 1).  `asked` is the nrhs the caller passed, checked by served().  The host forms of
// blocks (column-major on the host, relaid through a staging block) exist in ComplexF64 only.
int cx_block_ensure(mg_hierarchy* h, int nr);
struct CxCols {
  int nr;
  long long asked;
  static CxCols vec(long long nrhs = 1) { return {0, nrhs}; }
  static CxCols blk(long long nrhs) { return {(int)std::min<long long>(std::max<long long>(nrhs, 1), mgk::BLK_KMAX), nrhs}; }
  static CxCols of(int nr) { return {nr, std::max(nr, 1)}; }   // (inside the core: a count that was checked on the way in)
  const char* noun() const { return nr ? "block" : "vector"; }
  size_t len(long long n) const { return (size_t)n * (size_t)std::max(nr, 1); }
  DevBuf<double>& b(CxLevel& L) const { return nr ? L.Bb : L.b; }
  DevBuf<double>& r(CxLevel& L) const { return nr ? L.Br : L.r; }
  DevBuf<double>& x(CxLevel& L, int i) const { return nr ? L.Bx[i] : L.x[i]; }
  DevBuf<double>& stage_b(CxState& S) const { return nr ? S.Bstage_b : S.stage_b; }
  DevBuf<double>& stage_x(CxState& S) const { return nr ? S.Bstage_x : S.stage_x; }
  DevBuf<double>& cw_b(CxState& S) const { return nr ? S.Bcw_b : S.cw_b; }   // the widened coarsest pair of a CF32 handle
  DevBuf<double>& cw_x(CxState& S) const { return nr ? S.Bcw_x : S.cw_x; }
  DevBuf<double>& lu_work(CxState& S) const { return nr ? S.BluWork : S.luWork; }   // the triangular sweeps' work vector
  DevBuf<double>& relaxZ(CxLevel& L) const { return nr ? L.BrelaxZ : L.relaxZ; }    // the directions of the FGMRES relaxation
  DevBuf<double>& relaxAZ(CxLevel& L) const { return nr ? L.BrelaxAZ : L.relaxAZ; }
  DevBuf<double>& kZ(CxLevel& L) const { return nr ? L.BkZ : L.kZ; }
  DevBuf<double>& kAZ(CxLevel& L) const { return nr ? L.BkAZ : L.kAZ; }
  int served(mg_hierarchy* h) const;                                 // the column count, the schedule and the coarsest solve take it
  int ready(mg_hierarchy* h, long long n, CxWant want) const;        // + the handle, finalized, n = the fine level's rows
  int ensure(mg_hierarchy* h) const { return nr ? cx_block_ensure(h, nr) : MG_OK; }
  // host array -> dst (n values per column), enqueued on h's stream: one copy, for a block through `cm` and cx_relayout
  template <typename C>
  int upload(mg_hierarchy* h, const void* host, DevBuf<double>& cm, C* dst, long long n) const {
    const hipStream_t st = h->play->stream;
    if (nr == 0) {
      HIP_TRY(hipMemcpyAsync(dst, host, sizeof(C) * (size_t)n, hipMemcpyHostToDevice, st));
      return MG_OK;
    }
    if constexpr (std::is_same<C, cx_t>::value) {
      HIP_TRY(hipMemcpyAsync(cm.p, host, sizeof(cx_t) * len(n), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(mgk::cx_relayout<true>, dim3(cx_grid((long long)len(n))), dim3(mgk::BLK), 0, st, cxc(cm), dst, n, nr);
      HIP_TRY(hipGetLastError());
      return MG_OK;
    }
    return fail(MG_ERR_INVALID, "internal: host blocks are ComplexF64");
  }
  // src -> host array, enqueued the same way; the caller waits for the stream
  template <typename C>
  int download(mg_hierarchy* h, const C* src, DevBuf<double>& cm, void* host, long long n) const {
    const hipStream_t st = h->play->stream;
    if (nr == 0) {
      HIP_TRY(hipMemcpyAsync(host, src, sizeof(C) * (size_t)n, hipMemcpyDeviceToHost, st));
      return MG_OK;
    }
    if constexpr (std::is_same<C, cx_t>::value) {
      hipLaunchKernelGGL(mgk::cx_relayout<false>, dim3(cx_grid((long long)len(n))), dim3(mgk::BLK), 0, st, src, cxp(cm), n, nr);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(host, cm.p, sizeof(cx_t) * len(n), hipMemcpyDeviceToHost, st));
      return MG_OK;
    }
    return fail(MG_ERR_INVALID, "internal: host blocks are ComplexF64");
  }
};

// z = param.LU \ b (MGcycle.jl:177): explicit inverse, or x[q] = U \ (L \ b[p]) by the level-scheduled sptrsv_lu (one workgroup;
// chip-wide for factors of >= lu_multi_min_rows rows), or one Schwarz sweep (MGcycle.jl:140-143; xzero: x need not be read), or one
// restart of Jacobi-preconditioned FGMRES(10) from zero (cx_coarse_gmres: the only one that synchronises with the host, once)
// nr >= 1: b and x are row-major blocks [n][nr] (the factor applier's own layout; the Schwarz sweep serves one column)
int dd_coarse(mg_hierarchy* h, const cf_t* b, cf_t* x, bool x_zero);   // (mg_dd.inc: the sweep on a CF32 hierarchy's own coarsest vectors)
int cx_coarse(mg_hierarchy* h, const cx_t* b, cx_t* x, bool xzero = true, int nr = 0) {
  CxState& S = *h->cx;
  const long long n = S.n_coarse;
  const int k = std::max(nr, 1);
  if (h->coarse_dd) {
    if (k > 1) return fail(MG_ERR_UNSUPPORTED, "a Schwarz sweep as coarsest solve serves one right-hand side (nrhs=%d)", k);
    return dd_coarse(h, reinterpret_cast<const double*>(b), reinterpret_cast<double*>(x), xzero);
  }
  if (S.coarse_gmres) {   // (the reference calls blockFGMRES on a block, MGcycle.jl:166-167: served with the option coarse_gmres_blocks)
    if (k > 1 && !h->opt.coarse_gmres_blocks) return fail(MG_ERR_UNSUPPORTED, "the GMRES coarsest solve serves one right-hand side (nrhs=%d)", k);
    if (k > 1) return cx_coarse_block_gmres(h, b, x, k);
    return cx_coarse_gmres(h, b, x);   // (a block of one column is a vector)
  }
  if (S.coarse_multi) return cxlu_solve_dev(S.coarse_multi, *S.coarse_multi->fwd, b, x, k, &h->play->stream);
  if (S.coarse_lu) {
    mgk::LuDevT<cx_t> F;
    F.n = (int)n;
    F.Lptr = S.luLptr.p; F.Lcol = S.luLcol.p; F.Lval = reinterpret_cast<const cx_t*>(S.luLval.p);
    F.Uptr = S.luUptr.p; F.Ucol = S.luUcol.p; F.Uval = reinterpret_cast<const cx_t*>(S.luUval.p);
    F.p = S.luP.p; F.q = S.luQ.p;
    F.Lorder = S.luLorder.p; F.Llvl = S.luLlvl.p; F.nLlvl = S.nLlvl;
    F.Uorder = S.luUorder.p; F.Ulvl = S.luUlvl.p; F.nUlvl = S.nUlvl;
    hipLaunchKernelGGL(mgk::sptrsv_lu<cx_t>, dim3(1), dim3(1024), 0, h->play->stream, F, b, x, cxp(CxCols::of(nr).lu_work(S)), k);
  } else if (nr == 0) {
    hipLaunchKernelGGL(mgk::cx_dense_matvec, dim3(cx_grid(n * 64)), dim3(mgk::BLK), 0, h->play->stream,
                       reinterpret_cast<const cx_t*>(S.Ainv.p), b, x, (int)n);
  } else {
    hipLaunchKernelGGL(mgk::cx_dense_matblk, dim3(cx_grid(n * k * 64)), dim3(mgk::BLK), 0, h->play->stream,
                       reinterpret_cast<const cx_t*>(S.Ainv.p), b, x, (int)n, k);
  }
  HIP_TRY(hipGetLastError());
  return MG_OK;
}

// The coarsest solve of a CF32 handle stays ComplexF64 (Julia's lu of a ComplexF32 sparse matrix factorises in double,
// MGsetup.jl:350; MGcycle.jl:177-178): bc is widened, solved by the kernels above, xc narrowed.  The GMRES coarsest solve too: it runs
// in ComplexF64 on the widened copy of the coarsest operator (CxState::cgA).  The reference would run that fgmres in ComplexF32 - a
// deliberate deviation of the order of the single unit roundoff: more accurate, and no float instantiation of the vector passes.
int cx_coarse(mg_hierarchy* h, const cf_t* b, cf_t* x, bool xzero = true, int nr = 0) {
  CxState& S = *h->cx;
  // a ComplexF32 Schwarz sweep (mg_set_coarse_dd admits no other kind here): on the cycle's own bc and xc, no widened pair
  if (h->coarse_dd) {
    if (nr > 1) return fail(MG_ERR_UNSUPPORTED, "a Schwarz sweep as coarsest solve serves one right-hand side (nrhs=%d)", nr);
    return dd_coarse(h, b, x, xzero);
  }
  // ComplexF32 factors (mg_set_coarse_lu_CF32_INT64): applied to the cycle's own bc, no widened pair
  if (S.coarse_single) return cxlu_solve_dev(S.coarse_single, *S.coarse_single->fwd, b, x, std::max(nr, 1), &h->play->stream);
  const CxCols W = CxCols::of(nr);
  DevBuf<double>&wb = W.cw_b(S), &wx = W.cw_x(S);
  const long long len = (long long)W.len(S.n_coarse);
  MG_TRY(cx_widen(h, b, cxp(wb), len));
  MG_TRY(cx_coarse(h, cxc(wb), cxp(wx), true, nr));
  return cx_narrow(h, cxc(wx), x, len);
}

// relax (MGcycle.jl:122-136) entered with r = b - A x: numit-1 times {x += d.*r; r = b - A x}, then x += d.*r - i.e.
// max(numit, 1) sweeps x' = x + d.*(b - A x); from x = 0 the first one is x = d.*b.  x ping-pongs between L.x[0] / L.x[1].
// nr columns (0: a vector): d[row] is shared by the columns of a block.
template <typename C>
int cx_relax(mg_hierarchy* h, CxLevel& L, const C* b, int& xi, bool xzero, long long numit, int nr = 0) {
  const CxCols W = CxCols::of(nr);
  long long sweeps = std::max<long long>(numit, 1);
  if (xzero) {
    if (nr == 0)
      hipLaunchKernelGGL(mgk::cx_dscale<C>, dim3(cx_grid(L.n)), dim3(mgk::BLK), 0, h->play->stream, cxc<C>(L.d), b, cxp<C>(W.x(L, xi)), L.n);
    else
      hipLaunchKernelGGL(mgk::cx_dscale_blk<C>, dim3(cx_grid(L.n * nr)), dim3(mgk::BLK), 0, h->play->stream, cxc<C>(L.d), b,
                         cxp<C>(W.x(L, xi)), L.n * nr, nr);
    HIP_TRY(hipGetLastError());
    --sweeps;
  }
  for (long long s = 0; s < sweeps; ++s) {
    MG_TRY(cx_spmv<mgk::SMOOTH>(h, L.A, cxc<C>(W.x(L, xi)), cxp<C>(W.x(L, 1 - xi)), b, cxc<C>(L.d), nullptr, C{1, 0}, C{0, 0}, nr));
    xi = 1 - xi;
  }
  return MG_OK;
}

// relaxation type 2 (RelaxVankaFacesColor, MGcycle.jl:51-52, 99-100): numit Vanka iterations of x in place from the level's own CSR, none
// for a count of 0.  xzero: x was zero-filled by the caller, the from-zero pass opens the relaxation (mg_vanka.hpp).
// nr >= 1: b and x are row-major blocks of nr columns (option vanka_blocks), relaxed by the block form of the smoother.
template <typename C>
int cx_vanka_relax(mg_hierarchy* h, CxLevel& L, const C* b, C* x, long long numit, bool xzero, int nr = 0) {
  if (!L.vanka) return fail(MG_ERR_STATE, "a level has no Vanka blocks (mg_set_vanka_CF64 / _CF32)");
  if (nr != 0)
    return vanka_run_cx_blk<C>(L.vanka, L.A.rowptr.p, L.A.colidx.p, static_cast<const C*>(L.A.vals()), b, x, nr, numit, L.vanka_type, xzero,
                               h->play->stream);
  return vanka_run_cx<C>(L.vanka, L.A.rowptr.p, L.A.colidx.p, static_cast<const C*>(L.A.vals()), b, x, numit, L.vanka_type, xzero,
                         h->play->stream);
}

// ---- FGMRES_relaxation (FGMRES.jl:48-126): Jac-GMRES smoothing and the K-cycle, written once over the pair type C --------------------
// (C = cf_t, option single_kcycle: Z, AZ, the product and d.*w in single; the Gram scalars, the least squares and t in double.)
// One launch per direction (the GRAM epilogue of cx_csr_stream_spmv: w = A z_j, z_{j+1} = d.*w, the partials of column j of H and of
// xi[j]), one final sum over all scalars of the steps enqueued so far, one readback, ONE host synchronisation; the small least squares
// is host algebra (RelaxLsqC, mg_krylov_host.hpp).
static_assert(mgk::GRAM_MAXV == mgcv::MAXV, "the combination pass x += Z t takes all directions of a relaxation at once");
inline int cx_gram_slot(int j) { return 1 + j * j + 2 * j; }

// the relaxation's partials, scalars and pinned readback, for operators of up to `nblocks` row blocks
int cx_gram_ensure(mg_hierarchy* h, size_t nblocks) {
  CxState& S = *h->cx;
  const size_t need = std::max((size_t)CxState::GSCAL * nblocks, (size_t)mgcv::MAXS * mgcv::MAXB);
  if (S.gpart.n < need) {
    if (h->play->stream) HIP_TRY(spin_sync(h->play->stream));
    MG_TRY(S.gpart.alloc(need));
  }
  if (S.gscal.n == 0) MG_TRY(S.gscal.alloc((size_t)CxState::GSCAL));
  if (!S.h_gscal) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&S.h_gscal), sizeof(double) * CxState::GSCAL));
  return MG_OK;
}

// step j: w = A z into column j of AZ, znext = d.*w (null: the last direction, or a preconditioner that is a cycle)
// C: the pair type of the level (cx_t or cf_t), deduced from z
// nr >= 1: z, r0, znext and the columns of AZ are row-major blocks [n][nr] taken as long vectors (the block kernel; the same scalars)
template <typename C>
int cx_gram_step(mg_hierarchy* h, const CxLevel& L, const C* z, typename cx_non_deduced<C>::type* AZ, int j,
                 const typename cx_non_deduced<C>::type* r0, typename cx_non_deduced<C>::type* znext, int nr = 0) {
  CxState& S = *h->cx;
  const size_t ld = CxCols::of(nr).len(L.n);
  const CxMat& M = L.A;
  if (j < 0 || j >= mgk::GRAM_MAXV) return fail(MG_ERR_INVALID, "internal: direction %d of an FGMRES relaxation", j);
  if (S.gpart.n < (size_t)CxState::GSCAL * (size_t)M.nblocks) return fail(MG_ERR_STATE, "internal: the relaxation's partial sums are not sized");
  if (M.single != (sizeof(C) == sizeof(cf_t))) return fail(MG_ERR_INVALID, "internal: operator and vectors differ in precision");
  mgk::CxVecArgsT<C> v = {};
  v.x = z;
  v.y = AZ + (size_t)j * ld;
  v.d = cxc<C>(L.d);
  v.beta_zero = 1;
  v.az = AZ;
  v.ldz = (long long)ld;
  v.gj = j;
  v.r0 = r0;
  v.znext = znext;
  v.gpart = S.gpart.p + (size_t)cx_gram_slot(j) * (size_t)M.nblocks;
  if (nr < 0 || nr > mgk::BLK_KMAX) return fail(MG_ERR_INVALID, "internal: a block of %d columns", nr);
  if (M.wide) cx_launch<mgk::GRAM, long long, C, C>(h, M, M.rowptr64.p, v, nr);
  else cx_launch<mgk::GRAM, int, C, C>(h, M, M.rowptr.p, v, nr);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}

// the sums of the scalars [first, first + count) on the host: one final launch (a workgroup per scalar), one copy, one synchronisation
int cx_gram_read(mg_hierarchy* h, int first, int count, int nblocks, const double** out) {
  CxState& S = *h->cx;
  const hipStream_t st = h->play->stream;
  hipLaunchKernelGGL(mgkv::krv_final, dim3((unsigned)count), dim3(mgkv::KB), 0, st, S.gpart.p + (size_t)first * (size_t)nblocks, nblocks,
                     S.gscal.p + first);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(S.h_gscal + first, S.gscal.p + first, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, st));
  HIP_TRY(spin_sync(st));
  *out = S.h_gscal;
  return MG_OK;
}

// column j of H and xi[j] from the summed scalars of step j
inline void cx_gram_fill(RelaxLsqC& Q, int j, const double* s) {
  const double* g = s + cx_gram_slot(j);
  Q.set(j, j, std::complex<double>(g[0], 0.0));
  Q.xi[(size_t)j] = std::complex<double>(g[1], g[2]);
  for (int i = 0; i < j; ++i) Q.set(i, j, std::complex<double>(g[3 + 2 * i], g[4 + 2 * i]));
}

// x += sum_{j < used} t_j Z_j in one pass (mgcv::OpCGsUpdate with h = -t; its ||x||^2 partial lands in the relaxation's own buffer, unread)
// (cf_t: mgcv::OpCRelaxCombineF - complex64 x and Z, the sum of an element in double, rounded once on the store)
int cx_relax_combine(mg_hierarchy* h, const RelaxLsqC& Q, int used, const cf_t* Z, cf_t* x, long long n) {
  mgcv::OpCRelaxCombineF op;
  op.m = used;
  op.x = x;
  for (int j = 0; j < mgcv::MAXV; ++j) {
    const int jj = j < used ? j : 0;
    op.t[j] = j < used ? cx_t{Q.t()[(size_t)j].real(), Q.t()[(size_t)j].imag()} : cx_t{0.0, 0.0};
    op.z[j] = Z + (size_t)jj * (size_t)n;
  }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(mgcv::cxv_pass<mgcv::OpCRelaxCombineF>), dim3((unsigned)mgcv::cxv_grid(n)), dim3(mgcv::KB), 0, h->play->stream, op,
                     n, h->cx->gpart.p);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
int cx_relax_combine(mg_hierarchy* h, const RelaxLsqC& Q, int used, const cx_t* Z, cx_t* x, long long n) {
  mgcv::OpCGsUpdate op;
  op.m = used;
  op.w = x;
  for (int j = 0; j < mgcv::MAXV; ++j) {
    const int jj = j < used ? j : 0;
    op.h[j] = j < used ? cx_t{-Q.t()[(size_t)j].real(), -Q.t()[(size_t)j].imag()} : cx_t{0.0, 0.0};
    op.v[j] = Z + (size_t)jj * (size_t)n;
  }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(mgcv::cxv_pass<mgcv::OpCGsUpdate>), dim3((unsigned)mgcv::cxv_grid(n)), dim3(mgcv::KB), 0, h->play->stream, op, n,
                     h->cx->gpart.p);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}

// what a caller may ask back of one relaxation (mg_fgmres_relax_CF64)
struct CxRelaxReport {
  RelaxLsqC* Q = nullptr;
  double* rnorms = nullptr;   // `inner` entries; those behind `used` stay untouched
  int used = 0;
};

// FGMRES_relaxation with the diagonal preconditioner on L.A: x += Z t.  On entry column 0 of Z holds z_1 = d.*r0 and the partials of
// ||r0||^2 sit in scalar 0 (both left by the residual in front, or by cx_relax_front_zero when r0 = b).  All `inner` GRAM steps are
// enqueued back to back - step j + 1 needs w_j only, never t - and the host replays the reference's loop on the leading blocks of H:
// at step j the (j+1) x (j+1) solve, break at the first rn < tol (FGMRES.jl:114-117), used = j + 1.  Directions beyond `used` are
// not read (the reference's zero-padded H gives the same t).
// nr >= 1: r0, x and every direction are row-major blocks [n][nr], and the relaxation is the reference's long-vector form
// (FGMRES.jl:51-53, 89-97): ONE H, xi, t and break test for the whole block, so its columns are coupled.
template <typename C>
int cx_fgmres_relax(mg_hierarchy* h, const CxLevel& L, const C* r0, typename cx_non_deduced<C>::type* x, int inner, double tol,
                    typename cx_non_deduced<C>::type* Z, typename cx_non_deduced<C>::type* AZ, CxRelaxReport* report = nullptr, int nr = 0) {
  if (inner <= 0) return MG_OK;   // w = Z*t with no columns: x unchanged (FGMRES.jl:119-123)
  if (inner > mgk::GRAM_MAXV) return fail(MG_ERR_UNSUPPORTED, "an FGMRES relaxation of %d directions (at most %d)", inner, mgk::GRAM_MAXV);
  const size_t n = CxCols::of(nr).len(L.n);
  for (int j = 0; j < inner; ++j) MG_TRY(cx_gram_step(h, L, Z + (size_t)j * n, AZ, j, r0, j + 1 < inner ? Z + (size_t)(j + 1) * n : nullptr, nr));
  const double* s = nullptr;
  MG_TRY(cx_gram_read(h, 0, (inner + 1) * (inner + 1), L.A.nblocks, &s));
  const double rnorm0 = std::sqrt(s[0]);
  RelaxLsqC local(inner);
  RelaxLsqC& Q = (report && report->Q) ? *report->Q : local;
  int used = 0;
  for (int j = 0; j < inner; ++j) {
    cx_gram_fill(Q, j, s);
    const double rn = Q.step(j + 1, rnorm0);
    used = j + 1;
    if (report && report->rnorms) report->rnorms[j] = rn;
    if (rn < tol) break;
  }
  if (report) report->used = used;
  return cx_relax_combine(h, Q, used, Z, x, (long long)n);
}

// z_1 = d.*b with the partials of ||b||^2 (scalar 0): the front of a relaxation from x = 0, where r0 = b
// (nr >= 1: Z_1 = d.*B on a row-major block, the partials of ||B||_F^2)
template <typename C>
int cx_relax_front_zero(mg_hierarchy* h, const CxLevel& L, const C* b, typename cx_non_deduced<C>::type* Z, int nr = 0) {
  if (nr == 0)
    hipLaunchKernelGGL(mgk::cx_dscale_sumsq<C>, dim3((unsigned)L.A.nblocks), dim3(mgk::BLK), 0, h->play->stream, cxc<C>(L.d), b, Z, L.n, h->cx->gpart.p);
  else
    hipLaunchKernelGGL(mgk::cx_dscale_sumsq_blk<C>, dim3((unsigned)L.A.nblocks), dim3(mgk::BLK), 0, h->play->stream, cxc<C>(L.d), b, Z, L.n * nr, nr,
                       h->cx->gpart.p);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}

// recursiveCycle (MGcycle.jl:1-118) from level l (0-based) on b; the iterate is lev[l].x[xi] (zero on entry when xzero).
// C = cx_t on a CF64 handle, cf_t on a CF32 one: the same recursion on the same buffers.
// nr columns (0: a vector on the handle's own level vectors; >= 1: row-major blocks on the block work set, xzero a property of the
// whole block as norm(x) is in the reference).
template <typename C>
int cx_cycle(mg_hierarchy* h, int l, const C* b, int& xi, bool xzero, char ctype, int nr = 0) {
  CxState& S = *h->cx;
  const int nl = (int)h->nlevels;
  CxLevel& L = S.lev[(size_t)l];
  const CxCols W = CxCols::of(nr);
  const C one = C{1, 0}, zero = C{0, 0};
  if (l == nl - 1) return cx_coarse(h, b, cxp<C>(W.x(L, xi)), xzero, nr);                 // l.13-18
  constexpr bool is64 = sizeof(typename mgk::cx_scalar<C>::type) == sizeof(double);
  const bool gmres_relax = h->relax_type == 1;   // Jac-GMRES (MGcycle.jl:35-38, 48-50, 96-98)
  const double gmresTol = 1e-5;                  // l.5
  if ((gmres_relax || ctype == 'K') && ((!is64 && !h->opt.single_kcycle) || (nr != 0 && !h->opt.kcycle_blocks)))
    return fail(MG_ERR_UNSUPPORTED, "Jac-GMRES smoothing and the K-cycle serve CF64 handles (CF32 ones with the option single_kcycle) and one right-hand side");   // (blocks: the option kcycle_blocks)
  const bool vanka_relax = h->relax_type == 2;   // Vanka (l.51-52, 99-100): x relaxed in place, no ping-pong
  if (vanka_relax && nr != 0 && !h->opt.vanka_blocks) return fail(MG_ERR_UNSUPPORTED, "Vanka relaxation (type 2) serves one right-hand side");
  if (vanka_relax) {   // (a block, option vanka_blocks: the block form of the smoother on Bx, in place as well)
    C* x = cxp<C>(W.x(L, xi));
    if (xzero) HIP_TRY(hipMemsetAsync(x, 0, sizeof(C) * W.len(L.n), h->play->stream));
    MG_TRY(cx_vanka_relax<C>(h, L, b, x, L.npre, xzero, nr));
  } else if (gmres_relax) {
    // r = b - A x (l.28-31) with ||r||^2 and z_1 = d.*r from the same pass; from x = 0, r0 = b
    // (a block, option kcycle_blocks: the same on the block work set, the block one long vector)
    C* x = cxp<C>(W.x(L, xi));
    if (xzero) HIP_TRY(hipMemsetAsync(x, 0, sizeof(C) * W.len(L.n), h->play->stream));
    if (L.npre > 0) {
      if (xzero) MG_TRY(cx_relax_front_zero<C>(h, L, b, cxp<C>(W.relaxZ(L)), nr));
      else MG_TRY(cx_spmv<mgk::RESID>(h, L.A, (const C*)x, cxp<C>(W.r(L)), b, cxc<C>(L.d), S.gpart.p, one, zero, nr, cxp<C>(W.relaxZ(L))));
      MG_TRY(cx_fgmres_relax<C>(h, L, xzero ? b : cxc<C>(W.r(L)), x, (int)L.npre, gmresTol, cxp<C>(W.relaxZ(L)), cxp<C>(W.relaxAZ(L)), nullptr, nr));
    }
  } else {
    MG_TRY(cx_relax<C>(h, L, b, xi, xzero, L.npre, nr));                                  // l.26-31, 54
  }
  MG_TRY(cx_spmv<mgk::RESID>(h, L.A, cxc<C>(W.x(L, xi)), cxp<C>(W.r(L)), b, nullptr, nullptr, one, zero, nr));  // l.58-60
  CxLevel& C1 = S.lev[(size_t)l + 1];
  const C* bc = cxc<C>(W.b(C1));
  MG_TRY(cx_spmv<mgk::AXPBY>(h, L.R, cxc<C>(W.r(L)), cxp<C>(W.b(C1)), nullptr, nullptr, nullptr, one, zero, nr));   // bc = R r   (l.66)
  int ci = 0;
  if (l + 1 == nl - 1) {
    MG_TRY(cx_coarse(h, bc, cxp<C>(W.x(C1, ci)), true, nr));                         // l.67-69
  } else if (ctype == 'K') {
    // K-cycle (l.72-76): two FGMRES steps on A_{l+1} xc = bc from xc = 0, preconditioned by the K-cycle of level l+1 from zero.  Each
    // step: one inner cycle, its result copied into Z, one GRAM launch (no znext: the preconditioner is a cycle), one synchronisation -
    // so the break after step 1 costs no speculative sub-cycle.
    // (a block: the two steps on the long vector of length n1 * nr, the inner cycles on the whole block)
    const size_t n1 = W.len(C1.n);
    C *Z = cxp<C>(W.kZ(C1)), *AZ = cxp<C>(W.kAZ(C1));
    RelaxLsqC Q(2);
    double rnorm0 = 0.0;
    int used = 0;
    for (int j = 0; j < 2; ++j) {
      int cj = 0;
      MG_TRY(cx_cycle<C>(h, l + 1, j == 0 ? bc : (const C*)AZ, cj, true, 'K', nr));         // z = MMG(r0) / MMG(w)  (FGMRES.jl:83-87)
      HIP_TRY(hipMemcpyAsync(Z + (size_t)j * n1, W.x(C1, cj).p, sizeof(C) * n1, hipMemcpyDeviceToDevice, h->play->stream));
      if (j == 0) {                                                                         // rnorm0 = norm(r0)  (l.65)
        hipLaunchKernelGGL(mgk::cx_sumsq_partial<C>, dim3((unsigned)C1.A.nblocks), dim3(mgk::BLK), 0, h->play->stream, bc, (long long)n1, S.gpart.p);
        HIP_TRY(hipGetLastError());
      }
      MG_TRY(cx_gram_step<C>(h, C1, Z + (size_t)j * n1, AZ, j, bc, nullptr, nr));
      const double* s = nullptr;
      MG_TRY(cx_gram_read(h, j == 0 ? 0 : cx_gram_slot(1), j == 0 ? cx_gram_slot(1) : 5, C1.A.nblocks, &s));
      if (j == 0) rnorm0 = std::sqrt(s[0]);
      cx_gram_fill(Q, j, s);
      const double rn = Q.step(j + 1, rnorm0);
      used = j + 1;
      if (rn < gmresTol) break;                                                             // l.114-117
    }
    ci = 0;                                                                                 // xc = 0 + Z t  (l.121-123)
    HIP_TRY(hipMemsetAsync(W.x(C1, ci).p, 0, sizeof(C) * n1, h->play->stream));
    MG_TRY(cx_relax_combine(h, Q, used, Z, cxp<C>(W.x(C1, ci)), (long long)n1));
  } else {
    MG_TRY(cx_cycle<C>(h, l + 1, bc, ci, true, ctype, nr));                                // xc = 0 (l.63-64), l.78
    if (ctype == 'W') MG_TRY(cx_cycle<C>(h, l + 1, bc, ci, false, 'W', nr));               // l.79-80
    else if (ctype == 'F') MG_TRY(cx_cycle<C>(h, l + 1, bc, ci, false, 'V', nr));          // l.81-84
  }
  // x += P xc (l.90): in place, the gather reads xc only
  MG_TRY(cx_spmv<mgk::AXPBY>(h, L.P, cxc<C>(W.x(C1, ci)), cxp<C>(W.x(L, xi)), nullptr, nullptr, nullptr, one, one, nr));
  if (vanka_relax) return cx_vanka_relax<C>(h, L, b, cxp<C>(W.x(L, xi)), L.npost, false, nr);   // l.99-100
  if (gmres_relax) {                                                                      // r = b - A x, FGMRES_relaxation (l.92-98)
    if (L.npost > 0) {
      C* x = cxp<C>(W.x(L, xi));
      MG_TRY(cx_spmv<mgk::RESID>(h, L.A, (const C*)x, cxp<C>(W.r(L)), b, cxc<C>(L.d), S.gpart.p, one, zero, nr, cxp<C>(W.relaxZ(L))));
      MG_TRY(cx_fgmres_relax<C>(h, L, cxc<C>(W.r(L)), x, (int)L.npost, gmresTol, cxp<C>(W.relaxZ(L)), cxp<C>(W.relaxAZ(L)), nullptr, nr));
    }
    return MG_OK;
  }
  return cx_relax<C>(h, L, b, xi, false, L.npost, nr);                                   // r = b - A x, relax (l.92-102)
}

// The reference runs its FGMRES relaxation on a block as one long vector (FGMRES.jl:51): served where the handle's option
// kcycle_blocks is set (default 0: refused, as before that form existed; Vanka with 'K' stays refused either way).
int cx_block_schedule_ok(mg_hierarchy* h) {
  if ((h->cycle == 'K' || h->relax_type == 1) && (!h->opt.kcycle_blocks || h->relax_type == 2))
    return fail(MG_ERR_UNSUPPORTED, "blocks of right-hand sides are not served on a K-cycle / Jac-GMRES complex hierarchy");
  // (served by the block form of the smoother where the handle's option vanka_blocks is set; default 0: refused, as before it existed)
  if (h->relax_type == 2 && !h->opt.vanka_blocks) return fail(MG_ERR_UNSUPPORTED, "blocks of right-hand sides are not served on a complex Vanka hierarchy");
  return MG_OK;
}
// The reference calls blockFGMRES for a block on a GMRES coarsest solve (MGcycle.jl:166-167): cx_coarse_block_gmres, served where the
// handle's option coarse_gmres_blocks is set (default 0: refused, as before that solve existed).
int cx_block_coarse_ok(mg_hierarchy* h, long long nrhs) {
  if (h->cx->coarse_gmres && nrhs > 1 && !h->opt.coarse_gmres_blocks)
    return fail(MG_ERR_UNSUPPORTED, "blocks of right-hand sides are not served on a complex hierarchy with the GMRES coarsest solve (nrhs=%lld)", nrhs);
  return MG_OK;
}
int cx_block_nrhs_ok(long long nrhs) {
  if (nrhs < 1) return fail(MG_ERR_INVALID, "nrhs=%lld: a block holds at least one right-hand side", nrhs);
  if (nrhs > mgk::BLK_KMAX) return fail(MG_ERR_UNSUPPORTED, "complex blocks hold at most %d right-hand sides (nrhs=%lld)", mgk::BLK_KMAX, nrhs);
  return MG_OK;
}
// The checks of every entry point: a vector form takes nrhs = 1, a block form takes nrhs with each call (the handle's own nrhs stays 1)
int CxCols::served(mg_hierarchy* h) const {
  if (nr == 0) {
    if (asked != 1) return fail(MG_ERR_UNSUPPORTED, "complex handles serve one right-hand side (nrhs=%lld)", asked);
    return MG_OK;
  }
  MG_TRY(cx_block_nrhs_ok(asked));
  MG_TRY(cx_block_schedule_ok(h));
  return cx_block_coarse_ok(h, asked);
}
int CxCols::ready(mg_hierarchy* h, long long n, CxWant want) const {
  MG_TRY(cx_handle_ok(h, want));
  if (!h->cx->finalized) return fail(MG_ERR_STATE, "hierarchy not finalized: call mg_finalize first");
  MG_TRY(served(h));
  if (n != h->cx->lev[0].n) return fail(MG_ERR_INVALID, "n=%lld does not match the fine level (%lld rows)", n, h->cx->lev[0].n);
  if (h->coarse_dd && nr > 1) return fail(MG_ERR_UNSUPPORTED, "a Schwarz sweep as coarsest solve serves one right-hand side (nrhs=%lld)", asked);
  return MG_OK;
}

// The block work set for nr columns: allocated at the first block call, grown when a larger nr arrives (like CxKry::ensure), kept with
// the handle.  Nothing of the single-vector state is touched.
int cx_block_ensure(mg_hierarchy* h, int nr) {
  CxState& S = *h->cx;
  MG_TRY(cx_cb_ensure(h, nr));
  if (h->relax_type == 2) {   // Vanka levels (option vanka_blocks): the delta buffers of the block smoother, cells x bs x nr
    bool waited = false;
    for (auto& L : S.lev)
      if (L.vanka && L.vanka->bk < nr) {   // (also blocks bound again since the last block call)
        if (!waited) {
          (void)hipSetDevice(h->device);
          HIP_TRY(spin_sync(h->play->stream));
          waited = true;
        }
        MG_TRY(vanka_block_ensure(L.vanka, nr));
      }
  }
  // the direction blocks of the long-vector FGMRES relaxation (option kcycle_blocks), where the schedule needs them: per level with
  // Jac-GMRES max(npre, npost) blocks each of Z and AZ, per level with 'K' from level 2 on two blocks each (cx_finalize's counts)
  const int nl = (int)h->nlevels;
  const bool dirs = h->opt.kcycle_blocks;
  auto zlen = [&](int l, size_t kk) {
    const CxLevel& L = S.lev[(size_t)l];
    return (dirs && h->relax_type == 1 && l < nl - 1) ? (size_t)std::max(L.npre, L.npost) * cx_len(S, L.n) * kk : (size_t)0;
  };
  auto klen = [&](int l, size_t kk) {
    return (dirs && h->cycle == 'K' && l >= 1 && l < nl - 1) ? 2 * cx_len(S, S.lev[(size_t)l].n) * kk : (size_t)0;
  };
  if (nr <= S.blk_cap) {   // (the option may have been set since the work set was sized: then it is sized again, with the directions)
    bool sized = true;
    for (int l = 0; l < nl; ++l)
      sized = sized && S.lev[(size_t)l].BrelaxZ.n >= zlen(l, (size_t)S.blk_cap) && S.lev[(size_t)l].BkZ.n >= klen(l, (size_t)S.blk_cap);
    if (sized) return MG_OK;
    nr = S.blk_cap;
  }
  (void)hipSetDevice(h->device);
  HIP_TRY(spin_sync(h->play->stream));   // (an earlier block call may still read the buffers replaced below)
  S.blk_cap = 0;
  const size_t k = (size_t)nr;
  for (auto& L : S.lev) {
    const size_t len = cx_len(S, L.n) * k;
    for (DevBuf<double>* d : {&L.Bb, &L.Br, &L.Bx[0], &L.Bx[1]}) MG_TRY(d->alloc(len));
  }
  const size_t n0 = 2 * (size_t)S.lev[0].n * k, nc = 2 * (size_t)S.n_coarse * k;
  for (DevBuf<double>* d : {&S.Bstage_b, &S.Bstage_x, &S.Bstage_t}) MG_TRY(d->alloc(n0));
  if (S.single && !S.coarse_single && !h->coarse_dd) {   // (ComplexF32 factors are applied to the cycle's own block: no widened pair)
    MG_TRY(S.Bcw_b.alloc(nc));
    MG_TRY(S.Bcw_x.alloc(nc));
  } else {
    S.Bcw_b.release();
    S.Bcw_x.release();
  }
  for (int l = 0; l < nl; ++l) {
    CxLevel& L = S.lev[(size_t)l];
    for (DevBuf<double>* d : {&L.BrelaxZ, &L.BrelaxAZ}) {
      if (zlen(l, k) == 0) d->release();
      else MG_TRY(d->alloc(zlen(l, k)));
    }
    for (DevBuf<double>* d : {&L.BkZ, &L.BkAZ}) {
      if (klen(l, k) == 0) d->release();
      else MG_TRY(d->alloc(klen(l, k)));
    }
  }
  if (S.coarse_multi) {   // (no allocation inside the cycle: the factor applier's work vectors for nr columns)
    CxLu* F = S.coarse_multi;
    const size_t wlen = (size_t)S.n_coarse * k, tlen = (size_t)std::max(F->fwd->M, 1) * k;
    if (F->work.n < wlen) MG_TRY(F->work.alloc(wlen));
    if (F->tail.n < tlen) MG_TRY(F->tail.alloc(tlen));
  } else if (S.coarse_single) {
    CxLuT<cf_t>* F = S.coarse_single;
    const size_t wlen = (size_t)S.n_coarse * k, tlen = (size_t)std::max(F->fwd->M, 1) * k;
    if (F->work.n < wlen) MG_TRY(F->work.alloc(wlen));
    if (F->tail.n < tlen) MG_TRY(F->tail.alloc(tlen));
  } else if (S.coarse_lu) {
    MG_TRY(S.BluWork.alloc(nc));
  }
  S.blk_cap = nr;
  return MG_OK;
}

// A single (ComplexF32) operator A widened into K: the same pattern and row blocks (one chunk size for both precisions), the values
// through cx_widen.  Waited for.
int cx_widen_mat(mg_hierarchy* h, const CxMat& A, CxMat& K) {
  const hipStream_t st = h->play->stream;
  K.release();
  K.cplx = true;
  K.single = false;
  K.wide = A.wide;
  K.n_rows = A.n_rows; K.n_cols = A.n_cols; K.nnz = A.nnz; K.nblocks = A.nblocks; K.max_row = A.max_row;
  if (A.wide) {
    MG_TRY(K.rowptr64.alloc(A.rowptr64.n));
    HIP_TRY(hipMemcpyAsync(K.rowptr64.p, A.rowptr64.p, A.rowptr64.bytes(), hipMemcpyDeviceToDevice, st));
  } else {
    MG_TRY(K.rowptr.alloc(A.rowptr.n));
    HIP_TRY(hipMemcpyAsync(K.rowptr.p, A.rowptr.p, A.rowptr.bytes(), hipMemcpyDeviceToDevice, st));
  }
  MG_TRY(K.colidx.alloc(A.colidx.n));
  MG_TRY(K.blk_row.alloc(A.blk_row.n));
  MG_TRY(K.val.alloc(2 * (size_t)std::max<long long>(A.nnz, 1)));
  HIP_TRY(hipMemcpyAsync(K.colidx.p, A.colidx.p, A.colidx.bytes(), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(K.blk_row.p, A.blk_row.p, A.blk_row.bytes(), hipMemcpyDeviceToDevice, st));
  if (A.nnz > 0) MG_TRY(cx_widen(h, reinterpret_cast<const cf_t*>(A.valf.p), cxp(K.val), A.nnz));
  HIP_TRY(spin_sync(st));
  K.set = true;
  return MG_OK;
}

// the work set of the GMRES coarsest solve (no allocation inside a cycle), or nothing of it where another coarsest solve is set
int cx_cg_ensure(mg_hierarchy* h) {
  CxState& S = *h->cx;
  if (!S.coarse_gmres) {
    for (DevBuf<double>* d : {&S.cgD, &S.cgV, &S.cgZ, &S.cgTab, &S.cgPart}) d->release();
    S.cgA.release();
    return MG_OK;
  }
  const CxMat& Ac = S.lev.back().A;
  const size_t nc = (size_t)S.n_coarse;
  if (S.cgD.n != 2 * nc) return fail(MG_ERR_INVALID, "the coarsest Jacobi vector holds %zu values, the coarsest level %zu rows", S.cgD.n / 2, nc);
  if (h->play->stream) HIP_TRY(spin_sync(h->play->stream));
  const size_t vlen = 2 * nc * (mgcv::CG_M + 1), zlen = 2 * nc * mgcv::CG_M;
  const size_t plen = 4 * std::max<size_t>((size_t)Ac.nblocks, (size_t)mgcv::MAXB);
  if (S.cgV.n != vlen) MG_TRY(S.cgV.alloc(vlen));
  if (S.cgZ.n != zlen) MG_TRY(S.cgZ.alloc(zlen));
  if (S.cgTab.n != (size_t)mgcv::CG_TAB) MG_TRY(S.cgTab.alloc((size_t)mgcv::CG_TAB));
  if (S.cgPart.n != plen) MG_TRY(S.cgPart.alloc(plen));
  if (!S.h_cgtab) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&S.h_cgtab), sizeof(double) * mgcv::CG_TAB));
  if (S.single) MG_TRY(cx_widen_mat(h, Ac, S.cgA));   // (the level's values may have changed since the last finalize)
  else S.cgA.release();
  return MG_OK;
}

// mg_finalize of a CF64 handle: shapes chain, every level complete, scratch allocated
int cx_finalize(mg_hierarchy* h) {
  CxState& S = *h->cx;
  S.finalized = false;
  S.blk_cap = 0;   // (levels may have changed size: the block work set is sized again by the next block call)
  S.cb_cap = 0;
  const int nl = (int)h->nlevels;
  if (S.K_auto) {   // As[1] may have changed since it was widened: the next driver call widens it again
    S.K.release();
    S.K_auto = false;
  }
  // (the option single_kcycle lifts both refusals: the GRAM step, its front and its combination pass in single)
  if (S.single && !h->opt.single_kcycle && h->cycle == 'K') return fail(MG_ERR_UNSUPPORTED, "cycle 'K' is not served for CF32 handles");
  if (S.single && !h->opt.single_kcycle && h->relax_type == 1)
    return fail(MG_ERR_UNSUPPORTED, "relaxation type 1 (Jac-GMRES) is not served for CF32 handles");
  if (h->relax_type != 0 && h->relax_type != 1 && h->relax_type != 2)
    return fail(MG_ERR_UNSUPPORTED, "relaxation type %d is not served for complex handles", h->relax_type);
  size_t maxblocks = 1;
  for (int l = 0; l < nl; ++l) {
    CxLevel& L = S.lev[(size_t)l];
    if (!L.A.set) return fail(MG_ERR_STATE, "As[%d] was not set", l + 1);
    if (L.A.n_rows != L.A.n_cols) return fail(MG_ERR_INVALID, "As[%d] is not square", l + 1);
    if (L.A.single != S.single) return fail(MG_ERR_STATE, "As[%d] was set in another precision than the handle's", l + 1);
    L.n = L.A.n_rows;
    maxblocks = std::max(maxblocks, (size_t)L.A.nblocks);
    if (l < nl - 1) {
      if (!L.P.set || !L.R.set) return fail(MG_ERR_STATE, "Ps[%d]/Rs[%d] were not set", l + 1, l + 1);
      if (!L.relax_set) return fail(MG_ERR_STATE, "relaxPrecs[%d] was not set", l + 1);
      if (L.d.n != cx_len(S, L.n)) return fail(MG_ERR_INVALID, "relaxPrecs[%d] has length %zu, expected %lld", l + 1, L.d.n / (S.single ? 1 : 2), L.n);
      if (L.P.single != S.single || L.R.single != S.single)
        return fail(MG_ERR_STATE, "Ps[%d]/Rs[%d] were set in another precision than the handle's", l + 1, l + 1);
    }
  }
  for (int l = 0; l < nl - 1; ++l) {
    CxLevel& L = S.lev[(size_t)l];
    const long long nc = S.lev[(size_t)l + 1].A.n_rows;
    if (L.P.n_rows != L.n || L.P.n_cols != nc)
      return fail(MG_ERR_INVALID, "Ps[%d] is %lldx%lld, expected %lldx%lld", l + 1, L.P.n_rows, L.P.n_cols, L.n, nc);
    if (L.R.n_rows != nc || L.R.n_cols != L.n)
      return fail(MG_ERR_INVALID, "Rs[%d] is %lldx%lld, expected %lldx%lld", l + 1, L.R.n_rows, L.R.n_cols, nc, L.n);
  }
  if (h->relax_type == 2)   // Vanka: every relaxed level has blocks, built for its operator (the pointwise slot carries the sweep counts)
    for (int l = 0; l < nl - 1; ++l) {
      const CxLevel& L = S.lev[(size_t)l];
      if (!L.vanka)
        return fail(MG_ERR_STATE, "relaxation type 2 (Vanka) is set, but level %d has no blocks (mg_set_vanka_%s)", l + 1, S.single ? "CF32" : "CF64");
      if (L.vanka->G.N != L.n)
        return fail(MG_ERR_INVALID, "the Vanka blocks of level %d serve %d unknowns, As[%d] has %lld rows", l + 1, L.vanka->G.N, l + 1, L.n);
      if (L.A.wide) return fail(MG_ERR_UNSUPPORTED, "As[%d] holds 64-bit row pointers: not served by the Vanka smoother", l + 1);
      if (L.vanka->single != S.single) return fail(MG_ERR_STATE, "the Vanka blocks of level %d were bound in another precision than the handle's", l + 1);
    }
  if (S.K.set && S.K.n_rows != S.lev[0].n)
    return fail(MG_ERR_INVALID, "the Krylov operator has order %lld, As[1] %lld rows (clear it with mg_set_krylov_operator_CFP64_INT64(h, n, NULL, ...), finalize, then set a matching one)", S.K.n_rows, S.lev[0].n);
  if (!S.coarse_set) return fail(MG_ERR_STATE, "the coarsest solve was not set");
  if (S.n_coarse != S.lev[(size_t)nl - 1].n)
    return fail(MG_ERR_INVALID, "coarse solve order %lld != coarsest level size %lld", S.n_coarse, S.lev[(size_t)nl - 1].n);
  (void)hipSetDevice(h->device);
  for (auto& L : S.lev) {
    const size_t len = cx_len(S, L.n);
    if (L.b.n != len) MG_TRY(L.b.alloc(len));
    if (L.r.n != len) MG_TRY(L.r.alloc(len));
    if (L.x[0].n != len) MG_TRY(L.x[0].alloc(len));
    if (L.x[1].n != len) MG_TRY(L.x[1].alloc(len));
  }
  const size_t n0 = 2 * (size_t)S.lev[0].n;
  if (S.stage_b.n != n0) MG_TRY(S.stage_b.alloc(n0));
  if (S.partial.n < maxblocks) MG_TRY(S.partial.alloc(maxblocks));
  if (S.single && !S.coarse_single && !h->coarse_dd) {
    const size_t nc = 2 * (size_t)S.n_coarse;
    if (S.cw_b.n != nc) MG_TRY(S.cw_b.alloc(nc));
    if (S.cw_x.n != nc) MG_TRY(S.cw_x.alloc(nc));
  } else {   // (a CF64 handle, or ComplexF32 factors / a ComplexF32 Schwarz sweep applied to the cycle's own bc: no widened pair)
    S.cw_b.release();
    S.cw_x.release();
  }
  if (S.coarse_lu && !S.coarse_multi && !S.coarse_single && S.luWork.n != 2 * (size_t)S.n_coarse) MG_TRY(S.luWork.alloc(2 * (size_t)S.n_coarse));
  // FGMRESmem of the schedule (MGsetup.jl:186-214): memRelax for Jac-GMRES, memKcycle for the K-cycle; dropped when the schedule left them
  const bool gmres_relax = h->relax_type == 1, kcycle = h->cycle == 'K';
  for (int l = 0; l < nl; ++l) {
    CxLevel& L = S.lev[(size_t)l];
    const long long m = (gmres_relax && l < nl - 1) ? std::max(L.npre, L.npost) : 0;
    if (m > mgk::GRAM_MAXV)
      return fail(MG_ERR_UNSUPPORTED, "relaxPre / relaxPost = %lld on level %d: a complex Jac-GMRES relaxation takes at most %d directions", m, l + 1,
                  mgk::GRAM_MAXV);
    const size_t zlen = (size_t)m * cx_len(S, L.n), klen = (kcycle && l >= 1 && l < nl - 1) ? 2 * cx_len(S, L.n) : 0;
    for (DevBuf<double>* d : {&L.relaxZ, &L.relaxAZ}) {
      if (zlen == 0) d->release();
      else if (d->n != zlen) MG_TRY(d->alloc(zlen));
    }
    for (DevBuf<double>* d : {&L.kZ, &L.kAZ}) {
      if (klen == 0) d->release();
      else if (d->n != klen) MG_TRY(d->alloc(klen));
    }
  }
  if (gmres_relax || kcycle) MG_TRY(cx_gram_ensure(h, maxblocks));
  MG_TRY(cx_cg_ensure(h));
  S.finalized = true;
  return MG_OK;
}

// ---- the factor applier, written once over the stored value type V (cx_t, cf_t, float) -------------------------------------
template <typename V>
void cxlu_destroy(CxLuT<V>* S) {
  if (!S) return;
  (void)hipSetDevice(S->device);
  if (S->stream) (void)spin_sync(S->stream);
  delete S->fwd;
  delete S->adj;
  for (DevBuf<V>* d : {&S->work, &S->tail, &S->stage_b, &S->stage_x, &S->stage_t}) d->release();
  if (S->stream) (void)hipStreamDestroy(S->stream);
  delete S;
}

// Validate and upload one set of factors in parLU's layout (the checks and the form selection of
// mg_set_coarse_lu_FP64_INT64, sizeof(V) bytes per value in the traffic term of the trailing block's estimate).
template <typename V>
int cxlu_upload(CxLuT<V>* S, CxLuSetT<V>* F, const long long* Lptr, const long long* Lcol, const typename lu_store<V>::scalar* Lval,
                const long long* Uptr, const long long* Ucol, const typename lu_store<V>::scalar* Uval, const long long* p,
                const long long* q, const char* what) {
  const long long n = S->n;
  const size_t N = (size_t)n;
  std::vector<int> LP, LC, LO, LL, UP, UC, UO, UL, pp(N), qq(N);
  MG_TRY(lu_convert(n, Lptr, Lcol, true, LP, LC, LO, LL));
  MG_TRY(lu_convert(n, Uptr, Ucol, false, UP, UC, UO, UL));
  for (size_t i = 0; i < N; ++i) {
    if (p[i] < 1 || p[i] > n || q[i] < 1 || q[i] > n) return fail(MG_ERR_INVALID, "permutation entry out of range");
    pp[i] = (int)(p[i] - 1);
    qq[i] = (int)(q[i] - 1);
  }
  auto up_i = [&](DevBuf<int>& d, const std::vector<int>& v) -> int {
    MG_TRY(d.alloc(v.size()));
    HIP_TRY(hipMemcpy(d.p, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
    return MG_OK;
  };
  MG_TRY(up_i(F->Lptr, LP)); MG_TRY(up_i(F->Lcol, LC)); MG_TRY(up_i(F->Lorder, LO)); MG_TRY(up_i(F->Llvl, LL));
  MG_TRY(up_i(F->Uptr, UP)); MG_TRY(up_i(F->Ucol, UC)); MG_TRY(up_i(F->Uorder, UO)); MG_TRY(up_i(F->Ulvl, UL));
  MG_TRY(up_i(F->P, pp)); MG_TRY(up_i(F->Q, qq));
  MG_TRY(F->Lval.alloc(LC.size()));
  MG_TRY(F->Uval.alloc(UC.size()));
  HIP_TRY(hipMemcpy(F->Lval.p, Lval, LC.size() * sizeof(V), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(F->Uval.p, Uval, UC.size() * sizeof(V), hipMemcpyHostToDevice));
  F->nLlvl = (int)LL.size() - 1;
  F->nUlvl = (int)UL.size() - 1;
  F->multi = n >= S->opt.lu_multi_min_rows;
  F->M = 0;
  if (!F->multi) return MG_OK;
  // Size M of the trailing block: a level costs ~8 us of dependent latency whatever its width, the dense product
  // sizeof(V)*M^2/2 bytes of traffic per factor - the candidate with the smallest estimate
  // (the estimate, the slots and the inversion sequence of mg_set_coarse_lu_FP64_INT64, mg_cabi.inc: keep the two in step)
  const int cap = (int)std::min<long long>(S->opt.lu_dense_tail_max, n);
  int M = 0;
  double best = 0.0;
  std::vector<int> o, lp;
  for (int cand = 0; cand <= cap; cand = cand == 0 ? (int)std::max<long long>(S->opt.lu_dense_tail_min, 1) : cand * 2) {
    lu_levels(n, LP, LC, true, cand, o, lp);
    double est = 8e-6 * (double)(lp.size() - 1);
    lu_levels(n, UP, UC, false, cand, o, lp);
    est += 8e-6 * (double)(lp.size() - 1) + 2.0 * (0.5 * (double)sizeof(V)) * (double)cand * (double)cand / 4e12;
    if (cand == 0 || est < best) { best = est; M = cand; }
  }
  auto slots = [&](const std::vector<int>& P, bool lower, const std::vector<int>& order, DevBuf<int>& d) -> int {
    std::vector<int> sl(order.size() * 4);
    for (size_t t = 0; t < order.size(); ++t) {
      const int r = order[t];
      sl[4 * t] = r;
      sl[4 * t + 1] = lower ? P[(size_t)r] : P[(size_t)r] + 1;          // off-diagonal entries [s, e)
      sl[4 * t + 2] = lower ? P[(size_t)r + 1] - 1 : P[(size_t)r + 1];
      sl[4 * t + 3] = lower ? P[(size_t)r + 1] - 1 : P[(size_t)r];      // the diagonal entry
    }
    return up_i(d, sl);
  };
  lu_levels(n, LP, LC, true, M, o, F->Llvl_h);
  MG_TRY(slots(LP, true, o, F->Lslot));
  lu_levels(n, UP, UC, false, M, o, F->Ulvl_h);
  MG_TRY(slots(UP, false, o, F->Uslot));
  // the block is gathered and inverted in ComplexF64 whatever V is; a single factor's inverse is then rounded into V (X: its double form)
  auto invert = [&](bool lower, const DevBuf<int>& ptr, const DevBuf<int>& col, const DevBuf<V>& val, DevBuf<V>& inv) -> int {
    constexpr bool direct = std::is_same<V, cx_t>::value;
    const int ld = (M + 63) / 64 * 64;
    const size_t len = (size_t)ld * (size_t)ld;
    DevBuf<cx_t> D, X;
    int rc = D.alloc(len);
    if (rc == MG_OK) rc = inv.alloc(len);
    if (rc == MG_OK && !direct) rc = X.alloc(len);
    if (rc == MG_OK && hipMemsetAsync(D.p, 0, len * sizeof(cx_t), S->stream) != hipSuccess) rc = fail(MG_ERR_HIP, "hipMemsetAsync failed");
    if (rc == MG_OK) {
      cx_t* out = direct ? reinterpret_cast<cx_t*>(inv.p) : X.p;
      hipLaunchKernelGGL(mgk::cx_tri_gather_block<V>, dim3(cx_grid((long long)ld * 64)), dim3(mgk::BLK), 0, S->stream, ptr.p, col.p,
                         (const V*)val.p, (int)n - M, M, ld, D.p);
      const dim3 g((unsigned)(ld / mgk::CX_TRI_NB));
      if (lower) hipLaunchKernelGGL(mgk::cx_tri_inverse<true>, g, dim3(256), 0, S->stream, (const cx_t*)D.p, out, ld);
      else hipLaunchKernelGGL(mgk::cx_tri_inverse<false>, g, dim3(256), 0, S->stream, (const cx_t*)D.p, out, ld);
      if constexpr (!direct)
        hipLaunchKernelGGL(mgk::cx_tri_store<V>, dim3(cx_grid((long long)len)), dim3(mgk::BLK), 0, S->stream, (const cx_t*)X.p, inv.p, (long long)len);
      if (hipGetLastError() != hipSuccess || hipStreamSynchronize(S->stream) != hipSuccess) rc = fail(MG_ERR_HIP, "inversion of the trailing block failed");
    }
    D.release();
    X.release();
    return rc;
  };
  if (M > 0) {
    MG_TRY(invert(true, F->Lptr, F->Lcol, F->Lval, F->invL));
    MG_TRY(invert(false, F->Uptr, F->Ucol, F->Uval, F->invU));
  }
  F->M = M;
  if (S->opt.debug_format)
    std::fprintf(stderr, "[mgvcycle] %s LU (%s) n=%lld: dense trailing block %d, L %zu levels ahead of it (%d in all), U %zu behind it (%d)\n",
                 lu_store<V>::kind == 1 ? "complex" : lu_store<V>::kind == 3 ? "single complex" : "single real",
                 what, n, M, F->Llvl_h.size() - 1, F->nLlvl, F->Ulvl_h.size() - 1, F->nUlvl);
  return MG_OK;
}

// CSR (1-based) of the conjugate transpose (comps = 1: the transpose) of an n x n CSR (1-based) matrix; columns of every row come out
// ascending, so U^H is lower triangular with its diagonal last and L^H upper triangular with its diagonal first
template <typename T, int comps = 2>
void cx_adjoint_csr1(long long n, const std::vector<long long>& ptr, const std::vector<long long>& col, const std::vector<T>& val,
                     std::vector<long long>& tp, std::vector<long long>& tc, std::vector<T>& tv) {
  const size_t nnz = col.size();
  tc.resize(nnz);
  tv.resize(comps * nnz);
  std::vector<long long> cnt((size_t)n, 0);
  for (size_t k = 0; k < nnz; ++k) cnt[(size_t)col[k] - 1]++;
  tp.assign((size_t)n + 1, 1);
  for (long long c = 0; c < n; ++c) tp[(size_t)c + 1] = tp[(size_t)c] + cnt[(size_t)c];
  std::vector<long long> pos(tp.begin(), tp.end() - 1);
  for (long long r = 0; r < n; ++r)
    for (long long k = ptr[(size_t)r] - 1; k < ptr[(size_t)r + 1] - 1; ++k) {
      const long long c = col[(size_t)k] - 1;
      const long long w = pos[(size_t)c]++ - 1;
      tc[(size_t)w] = r + 1;
      tv[comps * (size_t)w] = val[comps * (size_t)k];
      if (comps == 2) tv[2 * (size_t)w + 1] = -val[2 * (size_t)k + 1];
    }
}

// the resident set of one solve direction; the adjoint set is built on its first use and kept beside the plain one
template <typename V>
int cxlu_set(CxLuT<V>* S, bool adjoint, CxLuSetT<V>** out) {
  CxLuSetT<V>*& F = adjoint ? S->adj : S->fwd;
  if (!F) {
    CxLuSetT<V>* G = new CxLuSetT<V>();
    int rc;
    if (!adjoint) {
      rc = cxlu_upload(S, G, S->Lptr.data(), S->Lcol.data(), S->Lval.data(), S->Uptr.data(), S->Ucol.data(), S->Uval.data(), S->p.data(),
                       S->q.data(), "plain");
    } else {   // A^H = Q U^H L^H P with A[p,q] = L U: x[p] = L^H \ (U^H \ b[q])
      typedef typename lu_store<V>::scalar T;
      std::vector<long long> lp, lc, up, uc;
      std::vector<T> lv, uv;
      cx_adjoint_csr1<T, lu_store<V>::comps>(S->n, S->Uptr, S->Ucol, S->Uval, lp, lc, lv);
      cx_adjoint_csr1<T, lu_store<V>::comps>(S->n, S->Lptr, S->Lcol, S->Lval, up, uc, uv);
      rc = cxlu_upload(S, G, lp.data(), lc.data(), lv.data(), up.data(), uc.data(), uv.data(), S->q.data(), S->p.data(), "adjoint");
    }
    if (rc != MG_OK) {
      delete G;
      return rc;
    }
    F = G;
  }
  *out = F;
  return MG_OK;
}

// x = A \ b (or A^H \ b) on device vectors, row-major [n][nrhs]; enqueued on S->stream (on: on *on, a borrower's stream), no
// synchronisation
template <typename V>
int cxlu_solve_dev(CxLuT<V>* S, CxLuSetT<V>& G, const V* b, V* x, int nr, const hipStream_t* on) {
  const hipStream_t st = on ? *on : S->stream;
  const long long n = S->n;
  const size_t wlen = (size_t)n * (size_t)nr, tlen = (size_t)std::max(G.M, 1) * (size_t)nr;
  if (S->work.n < wlen) MG_TRY(S->work.alloc(wlen));
  if (S->tail.n < tlen) MG_TRY(S->tail.alloc(tlen));
  mgk::LuDevT<V> F;
  F.n = (int)n;
  F.Lptr = G.Lptr.p; F.Lcol = G.Lcol.p; F.Lval = G.Lval.p;
  F.Uptr = G.Uptr.p; F.Ucol = G.Ucol.p; F.Uval = G.Uval.p;
  F.p = G.P.p; F.q = G.Q.p;
  F.Lorder = G.Lorder.p; F.Llvl = G.Llvl.p; F.nLlvl = G.nLlvl;
  F.Uorder = G.Uorder.p; F.Ulvl = G.Ulvl.p; F.nUlvl = G.nUlvl;
  V* y = S->work.p;
  if (!G.multi) {
    hipLaunchKernelGGL(mgk::sptrsv_lu<V>, dim3(1), dim3(1024), 0, st, F, b, x, y, nr);
    HIP_TRY(hipGetLastError());
    return MG_OK;
  }
  auto wave_blocks = [](long long waves) { return dim3(cx_grid(waves * 64)); };
  V* t = S->tail.p;
  const int M = G.M, n0 = (int)n - M, ld = (M + 63) / 64 * 64;
  // y = L \ b[p]: the levels ahead of the trailing block one launch each, the block through its inverse
  const int nLl = (int)G.Llvl_h.size() - 1, nUl = (int)G.Ulvl_h.size() - 1;
  for (int l = 0; l < nLl; ++l) {
    const int t0 = G.Llvl_h[(size_t)l], t1 = G.Llvl_h[(size_t)l + 1];
    hipLaunchKernelGGL((mgk::cx_sptrsv_level<true, V>), wave_blocks(t1 - t0), dim3(mgk::BLK), 0, st, F,
                       reinterpret_cast<const int4*>(G.Lslot.p), t0, t1, b, y, nr);
  }
  if (M > 0) {
    hipLaunchKernelGGL(mgk::cx_sptrsv_tail_rhs<V>, wave_blocks(M), dim3(mgk::BLK), 0, st, F, n0, b, (const V*)y, t, nr);
    hipLaunchKernelGGL((mgk::cx_tri_apply<true, V>), wave_blocks((long long)M * nr), dim3(mgk::BLK), 0, st,
                       (const V*)G.invL.p, ld, (const V*)t, y + (size_t)n0 * (size_t)nr, M, nr);
    // y = U \ y: the trailing block first, then the levels behind it
    HIP_TRY(hipMemcpyAsync(t, y + (size_t)n0 * (size_t)nr, (size_t)M * (size_t)nr * sizeof(V), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL((mgk::cx_tri_apply<false, V>), wave_blocks((long long)M * nr), dim3(mgk::BLK), 0, st,
                       (const V*)G.invU.p, ld, (const V*)t, y + (size_t)n0 * (size_t)nr, M, nr);
  }
  for (int l = 0; l < nUl; ++l) {
    const int t0 = G.Ulvl_h[(size_t)l], t1 = G.Ulvl_h[(size_t)l + 1];
    hipLaunchKernelGGL((mgk::cx_sptrsv_level<false, V>), wave_blocks(t1 - t0), dim3(mgk::BLK), 0, st, F,
                       reinterpret_cast<const int4*>(G.Uslot.p), t0, t1, b, y, nr);
  }
  hipLaunchKernelGGL(mgk::cx_sptrsv_scatter<V>, dim3(cx_grid(n * nr)), dim3(mgk::BLK), 0, st, (const int*)G.Q.p, (const V*)y, x, (int)n, nr);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}

// host form: b, x column-major n x nrhs in the handle's value type (complex: interleaved); b is only read
template <typename V>
int cxlu_solve_host(CxLuT<V>* S, CxLuSetT<V>& G, const typename lu_store<V>::scalar* b, typename lu_store<V>::scalar* x, int nr) {
  const long long n = S->n;
  const size_t len = (size_t)n * (size_t)nr, bytes = len * sizeof(V);
  if (S->stage_b.n < len) MG_TRY(S->stage_b.alloc(len));
  if (S->stage_x.n < len) MG_TRY(S->stage_x.alloc(len));
  if (nr > 1 && S->stage_t.n < len) MG_TRY(S->stage_t.alloc(len));
  if (nr == 1) {
    HIP_TRY(hipMemcpyAsync(S->stage_b.p, b, bytes, hipMemcpyHostToDevice, S->stream));
    MG_TRY(cxlu_solve_dev<V>(S, G, S->stage_b.p, S->stage_x.p, 1));
    HIP_TRY(hipMemcpyAsync(x, S->stage_x.p, bytes, hipMemcpyDeviceToHost, S->stream));
  } else {
    HIP_TRY(hipMemcpyAsync(S->stage_t.p, b, bytes, hipMemcpyHostToDevice, S->stream));
    hipLaunchKernelGGL((mgk::cx_relayout<true, V>), dim3(cx_grid(n * nr)), dim3(mgk::BLK), 0, S->stream, (const V*)S->stage_t.p, S->stage_b.p, n, nr);
    MG_TRY(cxlu_solve_dev<V>(S, G, S->stage_b.p, S->stage_x.p, nr));
    hipLaunchKernelGGL((mgk::cx_relayout<false, V>), dim3(cx_grid(n * nr)), dim3(mgk::BLK), 0, S->stream, (const V*)S->stage_x.p, S->stage_t.p, n, nr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(x, S->stage_t.p, bytes, hipMemcpyDeviceToHost, S->stream));
  }
  HIP_TRY(spin_sync(S->stream));
  return MG_OK;
}

// the create step behind mg_lu_create_*: arguments already checked for null / 1-based pointers
template <typename V>
int cxlu_create(long long device_id, long long n, const long long* Lptr, const long long* Lcol, const typename lu_store<V>::scalar* Lval,
                const long long* Uptr, const long long* Ucol, const typename lu_store<V>::scalar* Uval, const long long* p,
                const long long* q, CxLuT<V>** out, const Options* opt = nullptr) {
  constexpr int comps = lu_store<V>::comps;
  if (n >= (1LL << 31) - 1 || Lptr[n] - 1 >= (1LL << 31) || Uptr[n] - 1 >= (1LL << 31))
    return fail(MG_ERR_UNSUPPORTED, "factors exceed int32 device indices");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (ndev <= 0) return fail(MG_ERR_HIP, "no HIP device visible: the factor applier has no CPU fallback");
  if (device_id < 0 || device_id >= ndev) return fail(MG_ERR_INVALID, "device_id=%lld but %d devices visible", device_id, ndev);
  HIP_TRY(hipSetDevice((int)device_id));
  CxLuT<V>* S = new CxLuT<V>();
  S->opt = opt ? *opt : Options::from_env();   // the only place the environment is read for this handle (opt: a hierarchy's own)
  S->device = (int)device_id;
  S->n = n;
  S->Lptr.assign(Lptr, Lptr + n + 1);
  S->Uptr.assign(Uptr, Uptr + n + 1);
  S->Lcol.assign(Lcol, Lcol + (Lptr[n] - 1));
  S->Lval.assign(Lval, Lval + comps * (Lptr[n] - 1));
  S->Ucol.assign(Ucol, Ucol + (Uptr[n] - 1));
  S->Uval.assign(Uval, Uval + comps * (Uptr[n] - 1));
  S->p.assign(p, p + n);
  S->q.assign(q, q + n);
  int rc = MG_OK;
  if (hipStreamCreateWithFlags(&S->stream, hipStreamNonBlocking) != hipSuccess) rc = fail(MG_ERR_HIP, "hipStreamCreate failed");
  CxLuSetT<V>* F = nullptr;
  if (rc == MG_OK) rc = cxlu_set(S, false, &F);   // validates and uploads the factors
  if (rc != MG_OK) {
    cxlu_destroy(S);
    return rc;
  }
  *out = S;
  return MG_OK;
}


// ---- replaceMatrixInHierarchy on the device (mg_rap_CF64 and the value replacements) -------------------------------------
// column -> entries in ascending row order (stable counting sort of the stored pattern), for cx_colsumsq: build_transposed_pattern
// of the real operators, on a CxMat
int cx_build_transposed_pattern(CxMat& A) {
  if (A.wide) return fail(MG_ERR_UNSUPPORTED, "operators with 64-bit row pointers are not transposed on the device");
  if (A.has_t) return MG_OK;
  std::vector<int> rp((size_t)A.n_rows + 1), ci((size_t)std::max<long long>(A.nnz, 1));
  HIP_TRY(hipMemcpy(rp.data(), A.rowptr.p, rp.size() * sizeof(int), hipMemcpyDeviceToHost));
  if (A.nnz > 0) HIP_TRY(hipMemcpy(ci.data(), A.colidx.p, (size_t)A.nnz * sizeof(int), hipMemcpyDeviceToHost));
  std::vector<int> tp((size_t)A.n_cols + 1, 0), perm((size_t)std::max<long long>(A.nnz, 1));
  for (long long k = 0; k < A.nnz; ++k) ++tp[(size_t)ci[(size_t)k] + 1];
  for (long long j = 0; j < A.n_cols; ++j) tp[(size_t)j + 1] += tp[(size_t)j];
  std::vector<int> next(tp.begin(), tp.end() - 1);
  for (long long i = 0; i < A.n_rows; ++i)
    for (int k = rp[(size_t)i]; k < rp[(size_t)i + 1]; ++k) perm[(size_t)next[(size_t)ci[(size_t)k]]++] = k;
  MG_TRY(A.t_ptr.alloc(tp.size()));
  MG_TRY(A.t_perm.alloc(perm.size()));
  HIP_TRY(hipMemcpy(A.t_ptr.p, tp.data(), tp.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(A.t_perm.p, perm.data(), perm.size() * sizeof(int), hipMemcpyHostToDevice));
  A.has_t = true;
  return MG_OK;
}

template <typename VT>
mgk::CxCsr32<VT> cx_csr32(const CxMat& M) {
  return mgk::CxCsr32<VT>{M.rowptr.p, M.colidx.p, static_cast<const VT*>(M.vals())};   // (val, or valf of a CF32 handle's operator)
}

// New values on M's unchanged pattern from host memory, on h's stream and waited for: complex values arrive in the reference's
// AT convention and are conjugated in HBM (cx_conj), real ones are copied.
// ST: the host scalar, that of M's stored values (double, or float for the operators of a CF32 handle).
template <typename ST>
int cx_write_values(mg_hierarchy* h, CxMat& M, const ST* nzval) {
  constexpr bool single = sizeof(ST) == sizeof(float);
  if (M.single != single) return fail(MG_ERR_INVALID, "internal: values and operator differ in precision");
  const hipStream_t st = h->play->stream;
  HIP_TRY(spin_sync(st));
  if (M.nnz > 0) {
    HIP_TRY(hipMemcpyAsync(const_cast<void*>(M.vals()), nzval, (size_t)M.nnz * (M.cplx ? 2 : 1) * sizeof(ST), hipMemcpyHostToDevice, st));
    if (M.cplx) {
      if (single) hipLaunchKernelGGL(mgk::cx_conj32, dim3(cx_grid(M.nnz)), dim3(mgk::BLK), 0, st, reinterpret_cast<cf_t*>(M.valf.p), M.nnz);
      else hipLaunchKernelGGL(mgk::cx_conj, dim3(cx_grid(M.nnz)), dim3(mgk::BLK), 0, st, cxp(M.val), M.nnz);
    }
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(spin_sync(st));
  return MG_OK;
}

// The values of K, a widened copy of the single operator A made by cx_widen_mat on the pattern both still hold, widened again from
// A's present values: enqueued on h's stream, not waited for.
int cx_widen_values(mg_hierarchy* h, const CxMat& A, CxMat& K) {
  if (!K.set || K.single || !A.single || K.nnz != A.nnz || K.n_rows != A.n_rows)
    return fail(MG_ERR_STATE, "internal: the widened copy does not hold the operator's pattern");
  if (A.nnz > 0) MG_TRY(cx_widen(h, reinterpret_cast<const cf_t*>(A.valf.p), cxp(K.val), A.nnz));
  return MG_OK;
}

// the operator `which` of `level` of a CF64 handle (want: or of a CF32 one), set
int cx_find_op(mg_hierarchy* h, long long level, long long which, CxMat** out, CxWant want = CX_WANT64) {
  MG_TRY(cx_level_ok(h, level, want));
  if (which != MG_OP_A && which != MG_OP_P && which != MG_OP_R) return fail(MG_ERR_INVALID, "bad operator selector %lld", which);
  if (which != MG_OP_A && level == h->nlevels) return fail(MG_ERR_INVALID, "the coarsest level %lld has no transfer operators", level);
  CxLevel& L = h->cx->lev[(size_t)level - 1];
  CxMat* M = which == MG_OP_A ? &L.A : which == MG_OP_P ? &L.P : &L.R;
  if (!M->set) return fail(MG_ERR_STATE, "operator %lld of level %lld was not set", which, level);
  *out = M;
  return MG_OK;
}

// ---- the host-pointer forms of cycle / solve / spmv, once for both precisions (ST: the host scalar, C: the device pair) and for
//      vectors and blocks (CxCols; mg_block_*_CF64: Julia's column-major n x nrhs blocks, relaid at the boundary) ----
inline bool host_all_zero(const float* x, long long len) {
  for (long long i = 0; i < len; ++i)
    if (x[i] != 0.0f) return false;
  return true;
}

// b, x: n values per column on the host (a block: column-major n x nrhs, relaid at the boundary); W: the work set they run on
template <typename C, typename ST>
int cx_cycle_host(mg_hierarchy* h, const ST* b, ST* x, long long n, long long x_is_zero, CxWant want, CxCols W) {
  MG_TRY(W.ready(h, n, want));
  if (!b || !x) return fail(MG_ERR_INVALID, "null %s", W.noun());
  (void)hipSetDevice(h->device);
  MG_TRY(W.ensure(h));
  CxState& S = *h->cx;
  CxLevel& L0 = S.lev[0];
  bool xz = (x_is_zero == 1);
  if (x_is_zero < 0) xz = host_all_zero(x, 2 * (long long)W.len(n));   // norm(x) > 0.0 over the whole block decides (MGcycle.jl:29)
  int xi = 0;
  MG_TRY(W.upload(h, b, S.Bstage_t, cxp<C>(W.stage_b(S)), n));
  if (!xz) MG_TRY(W.upload(h, x, S.Bstage_t, cxp<C>(W.x(L0, xi)), n));
  MG_TRY(cx_cycle<C>(h, 0, cxc<C>(W.stage_b(S)), xi, xz, h->cycle, W.nr));
  MG_TRY(W.download(h, cxc<C>(W.x(L0, xi)), S.Bstage_t, x, n));
  HIP_TRY(spin_sync(h->play->stream));
  return MG_OK;
}

// solveMG (SolveFuncs.jl:14-36); on a block the norms are Frobenius norms of the whole block
template <typename C, typename ST>
int cx_solve_host(mg_hierarchy* h, const ST* b, ST* x, long long n, double tol, long long maxIter, long long* iters, double* resvec,
                  CxWant want, CxCols W) {
  MG_TRY(W.ready(h, n, want));
  if (!b || !x) return fail(MG_ERR_INVALID, "null %s", W.noun());
  if (maxIter < 0) return fail(MG_ERR_INVALID, "maxIter < 0");
  (void)hipSetDevice(h->device);
  MG_TRY(W.ensure(h));
  CxState& S = *h->cx;
  CxLevel& L0 = S.lev[0];
  const C* bd = cxc<C>(W.stage_b(S));
  int xi = 0;
  bool xz = host_all_zero(x, 2 * (long long)W.len(n));
  MG_TRY(W.upload(h, b, S.Bstage_t, cxp<C>(W.stage_b(S)), n));
  double res2 = 0.0;
  if (xz) {   // l.14-21
    MG_TRY(cx_norm2<C>(h, bd, (long long)W.len(n), &res2));
  } else {
    MG_TRY(W.upload(h, x, S.Bstage_t, cxp<C>(W.x(L0, xi)), n));
    MG_TRY(cx_residual_norm2<C>(h, L0, bd, cxc<C>(W.x(L0, xi)), cxp<C>(W.r(L0)), &res2, W.nr));
  }
  const double res0 = std::sqrt(res2);
  if (resvec) resvec[0] = res0;
  long long it = 0;
  for (long long count = 1; count <= maxIter; ++count) {   // l.23-37
    MG_TRY(cx_cycle<C>(h, 0, bd, xi, xz, h->cycle, W.nr));
    xz = false;
    MG_TRY(cx_residual_norm2<C>(h, L0, bd, cxc<C>(W.x(L0, xi)), cxp<C>(W.r(L0)), &res2, W.nr));
    ++it;
    const double res = std::sqrt(res2);
    if (resvec) resvec[count] = res;
    if (res / res0 < tol) break;
  }
  if (xz) HIP_TRY(hipMemsetAsync(W.x(L0, xi).p, 0, sizeof(C) * W.len(n), h->play->stream));   // maxIter = 0 from x = 0
  MG_TRY(W.download(h, cxc<C>(W.x(L0, xi)), S.Bstage_t, x, n));
  HIP_TRY(spin_sync(h->play->stream));
  if (iters) *iters = it;
  return MG_OK;
}

// y = beta*y + alpha*Op*x on one level; x holds n_cols and y n_rows values per column
template <typename C, typename ST>
int cx_spmv_host(mg_hierarchy* h, long long level, long long which, const ST* alpha, const ST* x, const ST* beta, ST* y, CxWant want,
                 CxCols W) {
  MG_TRY(cx_level_ok(h, level, want));
  CxState& S = *h->cx;
  if (!S.finalized) return fail(MG_ERR_STATE, "hierarchy not finalized");
  MG_TRY(W.served(h));
  if (!alpha || !beta || !x || !y) return fail(MG_ERR_INVALID, "null argument");
  if (which != MG_OP_A && which != MG_OP_P && which != MG_OP_R) return fail(MG_ERR_INVALID, "bad operator selector %lld", which);
  CxLevel& L = S.lev[(size_t)level - 1];
  if (which != MG_OP_A && level == h->nlevels) return fail(MG_ERR_INVALID, "the coarsest level %lld has no transfer operators", level);
  const CxMat& M = which == MG_OP_A ? L.A : which == MG_OP_P ? L.P : L.R;
  (void)hipSetDevice(h->device);
  const long long mr = M.n_rows, mc = M.n_cols;
  const C a = C{alpha[0], alpha[1]}, bt = C{beta[0], beta[1]};
  const bool bz = bt.x == 0 && bt.y == 0;
  DevBuf<double> cm, dx, dy;   // (released below on every path; cm: the column-major staging block of a block call)
  int rc = W.nr ? cm.alloc(2 * W.len(std::max(mr, mc))) : MG_OK;
  if (rc == MG_OK) rc = dx.alloc(cx_len(S, (long long)W.len(mc)));
  if (rc == MG_OK) rc = dy.alloc(cx_len(S, (long long)W.len(mr)));
  if (rc == MG_OK) rc = W.upload(h, x, cm, cxp<C>(dx), mc);
  if (rc == MG_OK && !bz) rc = W.upload(h, y, cm, cxp<C>(dy), mr);
  if (rc == MG_OK) rc = cx_spmv<mgk::AXPBY>(h, M, cxc<C>(dx), cxp<C>(dy), nullptr, nullptr, nullptr, a, bt, W.nr);
  if (rc == MG_OK) rc = W.download(h, cxc<C>(dy), cm, y, mr);
  if (spin_sync(h->play->stream) != hipSuccess && rc == MG_OK) rc = fail(MG_ERR_HIP, "mg_spmv: stream failed");
  cm.release();
  dx.release();
  dy.release();
  return rc;
}

// As[1] of a CF32 handle widened into the Krylov operator K: the system operator of the _CFP64 drivers when none was set (the
// Krylov product is never single).  Same pattern and row blocks (one chunk size for both precisions), values through cx_widen.
int cx_widen_K(mg_hierarchy* h) {
  CxState& S = *h->cx;
  MG_TRY(cx_widen_mat(h, S.lev[0].A, S.K));
  S.K_auto = true;
  return MG_OK;
}

// ---- adjointHierarchy on the device (mg_adjoint_hierarchy_CF64 / _CF32; MGsetup.jl:274-318 for complex VAL) -----------------
// the per-column ranking of cx_adj_order reads a column once per entry of it: longer columns are refused up front
constexpr int CX_ADJ_MAXCOL = 4096;

// what the host works out for one operator M before anything is written: the row pointers and row blocks of M'
struct CxAdjPlan {
  std::vector<int> tp, blk;
  long long max_row = 0;
};

// entries per column of M (cx_adj_count), read back and scanned; the row blocks by the rule of cx_upload.  Writes nothing of the handle.
int cx_adj_plan(mg_hierarchy* h, const CxMat& M, const char* what, int level, CxAdjPlan& plan) {
  const hipStream_t st = h->play->stream;
  const size_t m = (size_t)M.n_cols;
  DevBuf<int> cnt;
  plan.tp.assign(m + 1, 0);
  int rc = cnt.alloc(m);
  if (rc == MG_OK && hipMemsetAsync(cnt.p, 0, cnt.bytes(), st) != hipSuccess) rc = fail(MG_ERR_HIP, "hipMemsetAsync failed");
  if (rc == MG_OK && M.nnz > 0) {
    hipLaunchKernelGGL(mgk::cx_adj_count, dim3(cx_grid(M.nnz)), dim3(mgk::BLK), 0, st, M.colidx.p, (int)M.nnz, cnt.p);
    if (hipGetLastError() != hipSuccess) rc = fail(MG_ERR_HIP, "cx_adj_count failed to launch");
  }
  if (rc == MG_OK && (hipMemcpyAsync(plan.tp.data() + 1, cnt.p, m * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
                      spin_sync(st) != hipSuccess))
    rc = fail(MG_ERR_HIP, "readback of the column counts failed");
  cnt.release();
  MG_TRY(rc);
  plan.max_row = 0;
  for (size_t j = 0; j < m; ++j) {
    plan.max_row = std::max<long long>(plan.max_row, plan.tp[j + 1]);
    plan.tp[j + 1] += plan.tp[j];
  }
  if (plan.tp[m] != M.nnz) return fail(MG_ERR_HIP, "internal: the column counts of %s[%d] sum to %d, not %lld", what, level, plan.tp[m], M.nnz);
  if (plan.max_row > CX_ADJ_MAXCOL)
    return fail(MG_ERR_UNSUPPORTED, "%s[%d] holds a column of %lld entries: the per-column ordering of the device adjoint is quadratic (at most %d)", what,
                level, plan.max_row, CX_ADJ_MAXCOL);
  // row blocks: consecutive rows, <= MAXROWS rows and <= CX_CHUNK non-zeros (a longer row has a block of its own)
  const long long nr = M.n_cols;
  plan.blk.assign(1, 0);
  for (long long r = 0; r < nr;) {
    long long e = r + 1;
    while (e < nr && (e - r) < mgk::MAXROWS && plan.tp[(size_t)e + 1] - plan.tp[(size_t)r] <= mgk::CX_CHUNK) ++e;
    plan.blk.push_back((int)e);
    r = e;
  }
  return MG_OK;
}

// Out <- M' by the plan (Out may be M itself): new arrays are filled in HBM, then take the old ones' place.  VT: M's stored values.
template <typename VT>
int cx_adj_apply(mg_hierarchy* h, const CxMat& M, const CxAdjPlan& plan, CxMat& Out) {
  const hipStream_t st = h->play->stream;
  const size_t nnz1 = (size_t)std::max<long long>(M.nnz, 1);
  CxMat N;
  N.cplx = M.cplx;
  N.single = M.single;
  N.wide = false;
  N.n_rows = M.n_cols;
  N.n_cols = M.n_rows;
  N.nnz = M.nnz;
  N.nblocks = (int)plan.blk.size() - 1;
  N.max_row = plan.max_row;
  DevBuf<int> cursor, trow;
  const size_t scalars = nnz1 * (M.cplx ? 2 : 1);   // of M's precision
  int rc = N.rowptr.alloc(plan.tp.size());
  if (rc == MG_OK) rc = N.colidx.alloc(nnz1);
  if (rc == MG_OK) rc = N.blk_row.alloc(plan.blk.size());
  if (rc == MG_OK) rc = M.single ? N.valf.alloc(scalars) : N.val.alloc(scalars);
  if (rc == MG_OK) rc = cursor.alloc((size_t)M.n_cols);
  if (rc == MG_OK) rc = trow.alloc(nnz1);
  if (rc == MG_OK && (hipMemcpyAsync(N.rowptr.p, plan.tp.data(), plan.tp.size() * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess ||
                      hipMemcpyAsync(N.blk_row.p, plan.blk.data(), plan.blk.size() * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess ||
                      hipMemsetAsync(cursor.p, 0, cursor.bytes(), st) != hipSuccess))
    rc = fail(MG_ERR_HIP, "upload of the adjoint's row pointers failed");
  if (rc == MG_OK && M.nnz > 0) {
    const dim3 g(cx_grid(M.nnz)), b(mgk::BLK);
    hipLaunchKernelGGL(mgk::cx_adj_scatter, g, b, 0, st, M.rowptr.p, M.colidx.p, (int)M.n_rows, (int)M.nnz, N.rowptr.p, cursor.p, trow.p);
    hipLaunchKernelGGL(mgk::cx_adj_order<VT>, g, b, 0, st, M.rowptr.p, M.colidx.p, static_cast<const VT*>(M.vals()), (int)M.n_rows, (int)M.nnz,
                       N.rowptr.p, trow.p, N.colidx.p, static_cast<VT*>(const_cast<void*>(N.vals())));
    if (hipGetLastError() != hipSuccess) rc = fail(MG_ERR_HIP, "the adjoint kernels failed to launch");
  }
  if (spin_sync(st) != hipSuccess && rc == MG_OK) rc = fail(MG_ERR_HIP, "the adjoint of an operator failed on the device");   // (plan's arrays were read)
  cursor.release();
  trow.release();
  if (rc != MG_OK) {
    N.release();
    return rc;
  }
  N.set = true;
  Out.release();   // (with it the transposed pattern cached for SPAI re-setups: has_t / t_ptr / t_perm)
  Out = N;
  return MG_OK;
}

int cx_adj_apply(mg_hierarchy* h, const CxMat& M, const CxAdjPlan& plan, CxMat& Out) {
  if (M.cplx) return M.single ? cx_adj_apply<cf_t>(h, M, plan, Out) : cx_adj_apply<cx_t>(h, M, plan, Out);
  return M.single ? cx_adj_apply<float>(h, M, plan, Out) : cx_adj_apply<double>(h, M, plan, Out);
}

// As[l] <- As[l]', relaxPrecs[l] <- conj, Ps[l] <- Rs[l]' (Rs[l] keeps its values: the reference's literal pair of assignments), the
// coarsest solve for the adjoint operator, then the finalization path.  Every refusal precedes the first write.
int cx_adjoint_hierarchy(mg_hierarchy* h, CxWant want) {
  MG_TRY(cx_handle_ok(h, want));
  CxState& S = *h->cx;
  if (!S.finalized) return fail(MG_ERR_STATE, "hierarchy not finalized: call mg_finalize first");
  const int nl = (int)h->nlevels;
  for (int l = 0; l < nl; ++l) {
    const CxLevel& L = S.lev[(size_t)l];
    if (L.A.wide || (l + 1 < nl && (L.P.wide || L.R.wide)))
      return fail(MG_ERR_UNSUPPORTED, "level %d holds an operator with 64-bit row pointers: the device adjoint serves int32 operators (upload the adjoint hierarchy)", l + 1);
  }
  if (h->relax_type == 2) return fail(MG_ERR_UNSUPPORTED, "adjointHierarchy of a Vanka hierarchy is refused (MGsetup.jl:288-292)");
  if (S.coarse_lu) return fail(MG_ERR_UNSUPPORTED, "the coarsest solve is held as sparse factors: upload the adjoint hierarchy");
  if (h->coarse_dd) return fail(MG_ERR_UNSUPPORTED, "the coarsest solve is a Schwarz sweep (mg_set_coarse_dd): set the adjoint hierarchy up again");
  (void)hipSetDevice(h->device);
  const hipStream_t st = h->play->stream;
  HIP_TRY(spin_sync(st));
  std::vector<CxAdjPlan> planA((size_t)nl), planR((size_t)std::max(nl - 1, 0));
  for (int l = 0; l < nl; ++l) {
    MG_TRY(cx_adj_plan(h, S.lev[(size_t)l].A, "As", l + 1, planA[(size_t)l]));
    if (l + 1 < nl) MG_TRY(cx_adj_plan(h, S.lev[(size_t)l].R, "Rs", l + 1, planR[(size_t)l]));
  }
  // from here on a failure (allocation, HIP) leaves a partly flipped hierarchy: the handle is unfinalized first, so that every entry
  // point refuses it until the caller has uploaded again (the header says so)
  S.finalized = false;
  for (int l = 0; l < nl; ++l) {
    CxLevel& L = S.lev[(size_t)l];
    const auto t0 = std::chrono::steady_clock::now();
    MG_TRY(cx_adj_apply(h, L.A, planA[(size_t)l], L.A));   // (waited for: the host clock around it is the level's device time)
    if (h->opt.debug_format)
      std::fprintf(stderr, "[mgvcycle] adjoint As[%d]: %lld x %lld, %lld non-zeros, %d row blocks, %.3f ms\n", l + 1, L.A.n_rows, L.A.n_cols, L.A.nnz,
                   L.A.nblocks, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    if (l + 1 == nl) break;
    MG_TRY(cx_adj_apply(h, L.R, planR[(size_t)l], L.P));
    if (S.single) hipLaunchKernelGGL(mgk::cx_conj32, dim3(cx_grid(L.n)), dim3(mgk::BLK), 0, st, cxp<cf_t>(L.d), L.n);
    else hipLaunchKernelGGL(mgk::cx_conj, dim3(cx_grid(L.n)), dim3(mgk::BLK), 0, st, cxp(L.d), L.n);
    HIP_TRY(hipGetLastError());
  }
  const long long nc = S.n_coarse;
  if (S.coarse_gmres) {   // param.LU <- conj(param.LU)  (MGsetup.jl:304-305)
    hipLaunchKernelGGL(mgk::cx_conj, dim3(cx_grid(nc)), dim3(mgk::BLK), 0, st, cxp(S.cgD), nc);
  } else {                // (A')^-1 = (A^-1)'
    hipLaunchKernelGGL(mgk::cx_dense_adjoint_inplace, dim3(cx_grid(nc * nc)), dim3(mgk::BLK), 0, st, cxp(S.Ainv), (int)nc);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(spin_sync(st));
  // scratch sizes and shape checks again; a CF32 handle's widened coarsest operator (cgA) is rebuilt from the new As[end] and its
  // widened Krylov operator (K_auto) dropped, to be widened from the new As[1] by the next driver call
  return cx_finalize(h);
}

// mg_set_vanka_CF64 / _CF32: a VankaCore bound to a complex level, with the checks of mg_set_vanka_FP64
int cx_set_vanka(mg_hierarchy* h, long long level, CxWant want, long long dim, const long long* n, long long includePressure,
                 long long VankaType, const float* D_blocks) {
  UploadFence upload_fence;
  MG_TRY(cx_level_ok(h, level, want));
  CxLevel& L = h->cx->lev[(size_t)level - 1];
  if (!L.A.set) return fail(MG_ERR_STATE, "As[%lld] was not set: upload the operator before its Vanka blocks", level);
  if (L.A.wide) return fail(MG_ERR_UNSUPPORTED, "operators with 64-bit row pointers are not served by the Vanka smoother");
  if (L.A.n_rows != L.A.n_cols) return fail(MG_ERR_INVALID, "As[%lld] is not square", level);
  MG_TRY(vanka_type_served(VankaType));
  mgk::VankaGeo G;
  MG_TRY(vanka_geometry(dim, n, includePressure, L.A.n_rows, &G));
  (void)hipSetDevice(h->device);
  if (h->play->stream) HIP_TRY(spin_sync(h->play->stream));
  L.release_vanka();
  VankaCore* V = new VankaCore();
  const int rc = vanka_core_init(V, true, G, D_blocks, h->cx->single);
  if (rc != MG_OK) {
    V->release();
    delete V;
    return rc;
  }
  L.vanka = V;
  L.vanka_type = (int)VankaType;
  h->cx->finalized = false;
  return MG_OK;
}

// mg_build_vanka_CF64 / _CF32: cx_set_vanka with the blocks built in HBM from the level's resident operator (vanka_build_blocks,
// mg_vanka.hpp) for (VankaType, w[nw]), which the level remembers (mg_rap_CF64 with the option vanka_device_setup rebuilds from them).
// A singular cell: MG_ERR_INVALID, and the level keeps what it had.
int cx_build_vanka(mg_hierarchy* h, long long level, CxWant want, long long dim, const long long* n, long long includePressure,
                   long long VankaType, const double* w, long long nw) {
  UploadFence upload_fence;
  MG_TRY(cx_level_ok(h, level, want));
  CxLevel& L = h->cx->lev[(size_t)level - 1];
  if (!L.A.set) return fail(MG_ERR_STATE, "As[%lld] was not set: upload the operator before its Vanka blocks", level);
  if (L.A.wide) return fail(MG_ERR_UNSUPPORTED, "operators with 64-bit row pointers are not served by the Vanka smoother");
  if (L.A.n_rows != L.A.n_cols) return fail(MG_ERR_INVALID, "As[%lld] is not square", level);
  mgk::VankaBuild P;
  MG_TRY(vanka_build_args(VankaType, w, nw, &P));
  mgk::VankaGeo G;
  MG_TRY(vanka_geometry(dim, n, includePressure, L.A.n_rows, &G));
  (void)hipSetDevice(h->device);
  const hipStream_t st = h->play->stream;
  HIP_TRY(hipDeviceSynchronize());   // (the operator's upload ran on the NULL stream)
  VankaCore* V = new VankaCore();
  int bad = 0, first = 0;
  int rc = vanka_core_alloc(V, true, G, h->cx->single);
  if (rc == MG_OK) rc = vanka_build_launch(V, L.A.rowptr.p, L.A.colidx.p, L.A.vals(), P, st);
  if (rc == MG_OK && spin_sync(st) != hipSuccess) rc = fail(MG_ERR_HIP, "mg_build_vanka: the build failed on the device");
  if (rc == MG_OK) rc = vanka_build_finish(V, P, &bad, &first);
  if (rc == MG_OK && bad) rc = vanka_singular(bad, first, "mg_build_vanka");
  if (rc != MG_OK) {
    V->release();
    delete V;
    return rc;
  }
  L.release_vanka();
  L.vanka = V;
  L.vanka_type = (int)VankaType;
  h->cx->finalized = false;
  return MG_OK;
}

// mg_get_vanka_blocks_CF64 / _CF32: the level's blocks as mg_set_vanka_* takes them, count = bs*bs*cells ComplexF32 values
int cx_get_vanka_blocks(mg_hierarchy* h, long long level, CxWant want, float* out, long long count) {
  MG_TRY(cx_level_ok(h, level, want));
  if (!out) return fail(MG_ERR_INVALID, "null argument");
  CxLevel& L = h->cx->lev[(size_t)level - 1];
  if (!L.vanka) return fail(MG_ERR_STATE, "level %lld has no Vanka blocks", level);
  const long long have = (long long)L.vanka->G.bs * L.vanka->G.bs * L.vanka->G.cells;
  if (count != have) return fail(MG_ERR_INVALID, "count=%lld: level %lld holds %lld block values", count, level, have);
  (void)hipSetDevice(h->device);
  if (h->play->stream) HIP_TRY(spin_sync(h->play->stream));
  HIP_TRY(hipMemcpy(out, L.vanka->D.p, vanka_block_floats(L.vanka) * sizeof(float), hipMemcpyDeviceToHost));
  return MG_OK;
}

// mg_set_vanka_relax_CF64 / _CF32
int cx_set_vanka_relax(mg_hierarchy* h, CxWant want, long long cycleType) {
  MG_TRY(cx_handle_ok(h, want));
  if (cycleType != 'V' && cycleType != 'W' && cycleType != 'F' && cycleType != 'K')
    return fail(MG_ERR_INVALID, "cycleType must be 'V', 'W', 'F' or 'K'");
  h->cycle = (char)cycleType;   // ('K' on a CF32 handle: refused by mg_finalize unless the option single_kcycle is set)
  h->relax_type = 2;
  h->cx->finalized = false;
  return MG_OK;
}

// mg_create_CF64 / mg_create_CF32
int cx_create(long long nlevels, long long nrhs, long long device_id, mg_hierarchy** out, bool single) {
  if (!out) return fail(MG_ERR_INVALID, "out is null");
  *out = nullptr;
  if (nrhs != 1) return fail(MG_ERR_UNSUPPORTED, "complex handles serve one right-hand side (nrhs=%lld)", nrhs);
  mg_hierarchy* h = nullptr;
  MG_TRY(mg_create(nlevels, 1, device_id, &h));
  h->cx = new CxState();
  h->cx->single = single;
  h->cx->lev.resize((size_t)nlevels);
  *out = h;
  return MG_OK;
}

// FGMRES_relaxation with the diagonal preconditioner on one level, host vectors of the handle's precision (T: double or float, (re, im)
// interleaved): x += Z t.  Z_out / AZ_out (optional): the n x inner column-major bases of the relaxation.
template <typename C, typename T>
int cx_fgmres_relax_host(mg_hierarchy* h, long long level, const T* r0, T* x, long long n, long long inner, double tol, double* H_out,
                         double* xi_out, double* rnorms_out, long long* used_out, T* Z_out, T* AZ_out) {
  MG_TRY(cx_level_ok(h, level, sizeof(C) == sizeof(cf_t) ? CX_WANT32 : CX_WANT64));
  CxState& S = *h->cx;
  if (S.single && !h->opt.single_kcycle) return fail(MG_ERR_UNSUPPORTED, "mg_fgmres_relax_CF32 is not served for CF32 handles without the option single_kcycle");
  if (!S.finalized) return fail(MG_ERR_STATE, "hierarchy not finalized: call mg_finalize first");
  if (level >= h->nlevels) return fail(MG_ERR_INVALID, "level %lld holds no relaxPrecs (the coarsest level is solved, not relaxed)", level);
  if (inner < 1 || inner > mgk::GRAM_MAXV) return fail(MG_ERR_INVALID, "inner=%lld outside 1..%d", inner, mgk::GRAM_MAXV);
  if (!r0 || !x) return fail(MG_ERR_INVALID, "null vector");
  CxLevel& L = S.lev[(size_t)level - 1];
  if (n != L.n) return fail(MG_ERR_INVALID, "n=%lld does not match level %lld (%lld rows)", n, level, L.n);
  (void)hipSetDevice(h->device);
  MG_TRY(cx_gram_ensure(h, (size_t)L.A.nblocks));
  const hipStream_t st = h->play->stream;
  const int k = (int)inner;
  const size_t bytes = sizeof(C) * (size_t)n;
  DevBuf<double> dr, dx, dZ, dAZ;   // (released below on every path)
  RelaxLsqC Q(k);
  std::vector<double> rn((size_t)k, 0.0);
  CxRelaxReport report;
  report.Q = &Q;
  report.rnorms = rn.data();
  int rc = dr.alloc(cx_len(S, n));
  if (rc == MG_OK) rc = dx.alloc(cx_len(S, n));
  if (rc == MG_OK) rc = dZ.alloc(cx_len(S, n) * (size_t)k);
  if (rc == MG_OK) rc = dAZ.alloc(cx_len(S, n) * (size_t)k);
  if (rc == MG_OK && (hipMemcpyAsync(dr.p, r0, bytes, hipMemcpyHostToDevice, st) != hipSuccess ||
                      hipMemcpyAsync(dx.p, x, bytes, hipMemcpyHostToDevice, st) != hipSuccess))
    rc = fail(MG_ERR_HIP, "upload of r0 / x failed");
  if (rc == MG_OK) rc = cx_relax_front_zero<C>(h, L, cxc<C>(dr), cxp<C>(dZ));
  if (rc == MG_OK) rc = cx_fgmres_relax<C>(h, L, cxc<C>(dr), cxp<C>(dx), k, tol, cxp<C>(dZ), cxp<C>(dAZ), &report);
  if (rc == MG_OK && hipMemcpyAsync(x, dx.p, bytes, hipMemcpyDeviceToHost, st) != hipSuccess) rc = fail(MG_ERR_HIP, "download of x failed");
  if (rc == MG_OK && Z_out && hipMemcpyAsync(Z_out, dZ.p, bytes * (size_t)k, hipMemcpyDeviceToHost, st) != hipSuccess)
    rc = fail(MG_ERR_HIP, "download of Z failed");
  if (rc == MG_OK && AZ_out && hipMemcpyAsync(AZ_out, dAZ.p, bytes * (size_t)k, hipMemcpyDeviceToHost, st) != hipSuccess)
    rc = fail(MG_ERR_HIP, "download of AZ failed");
  if (spin_sync(st) != hipSuccess && rc == MG_OK) rc = fail(MG_ERR_HIP, "mg_fgmres_relax_%s: stream failed", sizeof(C) == sizeof(cf_t) ? "CF32" : "CF64");
  dr.release(); dx.release(); dZ.release(); dAZ.release();
  if (rc != MG_OK) return rc;
  for (int j = report.used; j < k; ++j) cx_gram_fill(Q, j, S.h_gscal);   // (the directions behind a break: summed, not used)
  if (H_out)
    for (int a = 0; a < k * k; ++a) {
      H_out[2 * a] = Q.H[(size_t)a].real();
      H_out[2 * a + 1] = Q.H[(size_t)a].imag();
    }
  if (xi_out)
    for (int a = 0; a < k; ++a) {
      xi_out[2 * a] = Q.xi[(size_t)a].real();
      xi_out[2 * a + 1] = Q.xi[(size_t)a].imag();
    }
  if (rnorms_out)
    for (int a = 0; a < k; ++a) rnorms_out[a] = a < report.used ? rn[(size_t)a] : 0.0;
  if (used_out) *used_out = report.used;
  return MG_OK;
}

// The same relaxation on a block of right-hand sides taken as one long vector (option kcycle_blocks; FGMRES.jl:51-53): R0, X and the
// bases are ComplexF64 column-major n x nrhs host blocks for both precisions (relaid to the device's row-major layout at the boundary;
// a CF32 handle narrows on the device and returns X, Z and AZ widened, which is exact).  Z_out / AZ_out (optional): n x nrhs x inner,
// of which the leading `used` blocks enter X.
template <typename C>
int cx_block_fgmres_relax_host(mg_hierarchy* h, long long level, const double* R0, double* X, long long n, long long nrhs, long long inner,
                               double tol, double* H_out, double* xi_out, double* rnorms_out, long long* used_out, double* Z_out,
                               double* AZ_out) {
  constexpr bool single = sizeof(C) == sizeof(cf_t);
  const char* name = single ? "mg_block_fgmres_relax_CF32" : "mg_block_fgmres_relax_CF64";
  MG_TRY(cx_level_ok(h, level, single ? CX_WANT32 : CX_WANT64));
  CxState& S = *h->cx;
  if (!h->opt.kcycle_blocks) return fail(MG_ERR_UNSUPPORTED, "%s is not served without the option kcycle_blocks", name);
  if (S.single && !h->opt.single_kcycle) return fail(MG_ERR_UNSUPPORTED, "%s is not served for CF32 handles without the option single_kcycle", name);
  if (!S.finalized) return fail(MG_ERR_STATE, "hierarchy not finalized: call mg_finalize first");
  if (level >= h->nlevels) return fail(MG_ERR_INVALID, "level %lld holds no relaxPrecs (the coarsest level is solved, not relaxed)", level);
  MG_TRY(cx_block_nrhs_ok(nrhs));
  if (inner > mgk::GRAM_MAXV) return fail(MG_ERR_UNSUPPORTED, "an FGMRES relaxation of %lld directions (at most %d)", inner, mgk::GRAM_MAXV);
  if (inner < 1) return fail(MG_ERR_INVALID, "inner=%lld outside 1..%d", inner, mgk::GRAM_MAXV);
  if (!R0 || !X) return fail(MG_ERR_INVALID, "null block");
  CxLevel& L = S.lev[(size_t)level - 1];
  if (n != L.n) return fail(MG_ERR_INVALID, "n=%lld does not match level %lld (%lld rows)", n, level, L.n);
  (void)hipSetDevice(h->device);
  MG_TRY(cx_gram_ensure(h, (size_t)L.A.nblocks));
  const hipStream_t st = h->play->stream;
  const int k = (int)inner, nr = (int)nrhs;
  const CxCols W = CxCols::of(nr);
  const size_t len = W.len(n), dlen = cx_len(S, n) * (size_t)nr;
  DevBuf<double> dr, dx, dZ, dAZ, cm, rm;   // (released below on every path; cm / rm: one column-major and one row-major ComplexF64 block)
  RelaxLsqC Q(k);
  std::vector<double> rn((size_t)k, 0.0);
  CxRelaxReport report;
  report.Q = &Q;
  report.rnorms = rn.data();
  // host block -> dst (the handle's precision, row-major), and back
  auto up = [&](const double* host, DevBuf<double>& dst) -> int {
    MG_TRY(W.upload<cx_t>(h, host, cm, single ? cxp(rm) : cxp(dst), n));
    if (single) MG_TRY(cx_narrow(h, cxc(rm), cxp<cf_t>(dst), (long long)len));
    return MG_OK;
  };
  auto down = [&](const C* src, double* host) -> int {
    if constexpr (single) {
      MG_TRY(cx_widen(h, src, cxp(rm), (long long)len));
      return W.download<cx_t>(h, cxc(rm), cm, host, n);
    } else {
      return W.download<cx_t>(h, src, cm, host, n);
    }
  };
  int rc = dr.alloc(dlen);
  if (rc == MG_OK) rc = dx.alloc(dlen);
  if (rc == MG_OK) rc = dZ.alloc(dlen * (size_t)k);
  if (rc == MG_OK) rc = dAZ.alloc(dlen * (size_t)k);
  if (rc == MG_OK) rc = cm.alloc(2 * len);
  if (rc == MG_OK) rc = rm.alloc(2 * len);
  if (rc == MG_OK) rc = up(R0, dr);
  if (rc == MG_OK) rc = up(X, dx);
  if (rc == MG_OK) rc = cx_relax_front_zero<C>(h, L, cxc<C>(dr), cxp<C>(dZ), nr);
  if (rc == MG_OK) rc = cx_fgmres_relax<C>(h, L, cxc<C>(dr), cxp<C>(dx), k, tol, cxp<C>(dZ), cxp<C>(dAZ), &report, nr);
  if (rc == MG_OK) rc = down(cxc<C>(dx), X);
  for (int j = 0; j < k && rc == MG_OK && Z_out; ++j) rc = down(cxc<C>(dZ) + (size_t)j * len, Z_out + 2 * (size_t)j * len);
  for (int j = 0; j < k && rc == MG_OK && AZ_out; ++j) rc = down(cxc<C>(dAZ) + (size_t)j * len, AZ_out + 2 * (size_t)j * len);
  if (spin_sync(st) != hipSuccess && rc == MG_OK) rc = fail(MG_ERR_HIP, "%s: stream failed", name);
  for (DevBuf<double>* d : {&dr, &dx, &dZ, &dAZ, &cm, &rm}) d->release();
  if (rc != MG_OK) return rc;
  for (int j = report.used; j < k; ++j) cx_gram_fill(Q, j, S.h_gscal);   // (the directions behind a break: summed, not used)
  if (H_out)
    for (int a = 0; a < k * k; ++a) {
      H_out[2 * a] = Q.H[(size_t)a].real();
      H_out[2 * a + 1] = Q.H[(size_t)a].imag();
    }
  if (xi_out)
    for (int a = 0; a < k; ++a) {
      xi_out[2 * a] = Q.xi[(size_t)a].real();
      xi_out[2 * a + 1] = Q.xi[(size_t)a].imag();
    }
  if (rnorms_out)
    for (int a = 0; a < k; ++a) rnorms_out[a] = a < report.used ? rn[(size_t)a] : 0.0;
  if (used_out) *used_out = report.used;
  return MG_OK;
}

}  // namespace

// =================================================================================================
// C ABI: the CF64 entry points
// =================================================================================================
extern "C" {

int mg_create_CF64(long long nlevels, long long nrhs, long long device_id, mg_hierarchy** out) {
  return cx_create(nlevels, nrhs, device_id, out, false);
}
int mg_create_CF32(long long nlevels, long long nrhs, long long device_id, mg_hierarchy** out) {
  return cx_create(nlevels, nrhs, device_id, out, true);
}

int mg_set_operator_CF64_INT64(mg_hierarchy* h, long long level, long long which, long long n_rows, long long n_cols,
                               const long long* colptr, const long long* rowval, const double* nzval) {
  UploadFence upload_fence;
  MG_TRY(cx_level_ok(h, level));
  if (which != MG_OP_A)
    return fail(MG_ERR_INVALID, "mg_set_operator_CF64_INT64 takes MG_OP_A only: P and R stay real (mg_set_operator_FP64_INT64)");
  (void)hipSetDevice(h->device);
  MG_TRY(cx_upload(&h->cx->lev[(size_t)level - 1].A, h->opt, n_rows, n_cols, colptr, rowval, nzval, true));
  h->cx->finalized = false;
  return MG_OK;
}

int mg_set_relax_CF64(mg_hierarchy* h, long long level, const double* d, long long n, long long relaxPre, long long relaxPost) {
  UploadFence upload_fence;
  MG_TRY(cx_level_ok(h, level));
  if (!d || n < 1) return fail(MG_ERR_INVALID, "empty relaxPrec");
  if (relaxPre < 0 || relaxPost < 0) return fail(MG_ERR_INVALID, "negative sweep count");
  (void)hipSetDevice(h->device);
  CxLevel& L = h->cx->lev[(size_t)level - 1];
  MG_TRY(L.d.alloc(2 * (size_t)n));
  HIP_TRY(hipMemcpy(L.d.p, d, 2 * (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  L.relax_set = true;
  L.npre = relaxPre;
  L.npost = relaxPost;
  h->cx->finalized = false;
  return MG_OK;
}

// cycleType and relaxType of a CF64 handle in one call: the K-cycle and Jac-GMRES smoothing arrive here (the shared setters
// mg_set_cycle_type / mg_set_relax_type keep refusing them on complex handles)
int mg_set_schedule_CF64(mg_hierarchy* h, long long cycleType, long long relaxType) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  if (!h->cx) return fail(MG_ERR_STATE, "CF64 entry point called on an FP64 handle (create it with mg_create_CF64)");
  MG_CF32_UNSUPPORTED(h);
  if (cycleType != 'V' && cycleType != 'W' && cycleType != 'F' && cycleType != 'K')
    return fail(MG_ERR_INVALID, "cycleType must be 'V', 'W', 'F' or 'K'");
  if (relaxType != 0 && relaxType != 1) return fail(MG_ERR_INVALID, "relaxType must be 0 (Jac / SPAI) or 1 (Jac-GMRES) on a CF64 handle");
  h->cycle = (char)cycleType;
  h->relax_type = (int)relaxType;
  h->cx->finalized = false;
  return MG_OK;
}
// The same for a CF32 handle whose option single_kcycle is set (MG_ERR_UNSUPPORTED without it)
int mg_set_schedule_CF32(mg_hierarchy* h, long long cycleType, long long relaxType) {
  MG_TRY(cx_handle_ok(h, CX_WANT32));
  if (!h->opt.single_kcycle) return fail(MG_ERR_UNSUPPORTED, "mg_set_schedule_CF32 is not served for CF32 handles without the option single_kcycle");
  if (cycleType != 'V' && cycleType != 'W' && cycleType != 'F' && cycleType != 'K')
    return fail(MG_ERR_INVALID, "cycleType must be 'V', 'W', 'F' or 'K'");
  if (relaxType != 0 && relaxType != 1) return fail(MG_ERR_INVALID, "relaxType must be 0 (Jac / SPAI) or 1 (Jac-GMRES) on a CF32 handle");
  h->cycle = (char)cycleType;
  h->relax_type = (int)relaxType;
  h->cx->finalized = false;
  return MG_OK;
}

// The Vanka blocks of one level of a complex handle (relaxation type 2): see include/mgvcycle.h
int mg_set_vanka_CF64(mg_hierarchy* h, long long level, long long dim, const long long* n, long long includePressure, long long VankaType,
                      const float* D_blocks) {
  return cx_set_vanka(h, level, CX_WANT64, dim, n, includePressure, VankaType, D_blocks);
}
int mg_set_vanka_CF32(mg_hierarchy* h, long long level, long long dim, const long long* n, long long includePressure, long long VankaType,
                      const float* D_blocks) {
  return cx_set_vanka(h, level, CX_WANT32, dim, n, includePressure, VankaType, D_blocks);
}

// The same with the blocks built on the device from the level's resident operator, and their readback: see include/mgvcycle.h
int mg_build_vanka_CF64(mg_hierarchy* h, long long level, long long dim, const long long* n, long long includePressure, long long VankaType,
                        const double* w, long long nw) {
  return cx_build_vanka(h, level, CX_WANT64, dim, n, includePressure, VankaType, w, nw);
}
int mg_build_vanka_CF32(mg_hierarchy* h, long long level, long long dim, const long long* n, long long includePressure, long long VankaType,
                        const double* w, long long nw) {
  return cx_build_vanka(h, level, CX_WANT32, dim, n, includePressure, VankaType, w, nw);
}
int mg_get_vanka_blocks_CF64(mg_hierarchy* h, long long level, float* out, long long count) {
  return cx_get_vanka_blocks(h, level, CX_WANT64, out, count);
}
int mg_get_vanka_blocks_CF32(mg_hierarchy* h, long long level, float* out, long long count) {
  return cx_get_vanka_blocks(h, level, CX_WANT32, out, count);
}

// Relaxation type 2 with its cycle type, on a complex handle (the shared setters and mg_set_schedule_CF64 keep refusing type 2)
int mg_set_vanka_relax_CF64(mg_hierarchy* h, long long cycleType) { return cx_set_vanka_relax(h, CX_WANT64, cycleType); }
int mg_set_vanka_relax_CF32(mg_hierarchy* h, long long cycleType) { return cx_set_vanka_relax(h, CX_WANT32, cycleType); }

// FGMRES_relaxation with the diagonal preconditioner on one level, host vectors: x += Z t
int mg_fgmres_relax_CF64(mg_hierarchy* h, long long level, const double* r0, double* x, long long n, long long inner, double tol,
                         double* H_out, double* xi_out, double* rnorms_out, long long* used_out) {
  return cx_fgmres_relax_host<cx_t, double>(h, level, r0, x, n, inner, tol, H_out, xi_out, rnorms_out, used_out, nullptr, nullptr);
}
// The same on a CF32 handle (option single_kcycle): complex64 vectors, the product in single, H / xi / rnorms in double; Z_out / AZ_out
// (optional) receive the n x inner column-major complex64 bases
int mg_fgmres_relax_CF32(mg_hierarchy* h, long long level, const float* r0, float* x, long long n, long long inner, double tol,
                         double* H_out, double* xi_out, double* rnorms_out, long long* used_out, float* Z_out, float* AZ_out) {
  return cx_fgmres_relax_host<cf_t, float>(h, level, r0, x, n, inner, tol, H_out, xi_out, rnorms_out, used_out, Z_out, AZ_out);
}

// The same relaxation on a block of right-hand sides as ONE long vector (option kcycle_blocks): see include/mgvcycle.h
int mg_block_fgmres_relax_CF64(mg_hierarchy* h, long long level, const double* R0, double* X, long long n, long long nrhs, long long inner,
                               double tol, double* H_out, double* xi_out, double* rnorms_out, long long* used_out, double* Z_out,
                               double* AZ_out) {
  return cx_block_fgmres_relax_host<cx_t>(h, level, R0, X, n, nrhs, inner, tol, H_out, xi_out, rnorms_out, used_out, Z_out, AZ_out);
}
int mg_block_fgmres_relax_CF32(mg_hierarchy* h, long long level, const double* R0, double* X, long long n, long long nrhs, long long inner,
                               double tol, double* H_out, double* xi_out, double* rnorms_out, long long* used_out, double* Z_out,
                               double* AZ_out) {
  return cx_block_fgmres_relax_host<cf_t>(h, level, R0, X, n, nrhs, inner, tol, H_out, xi_out, rnorms_out, used_out, Z_out, AZ_out);
}

// A of a CF32 handle from interleaved (re, im) float pairs (the reference's AT values, conjugated here once), P and R from floats
int mg_set_operator_CF32_INT64(mg_hierarchy* h, long long level, long long which, long long n_rows, long long n_cols,
                               const long long* colptr, const long long* rowval, const float* nzval) {
  UploadFence upload_fence;
  MG_TRY(cx_level_ok(h, level, CX_WANT32));
  if (which != MG_OP_A && which != MG_OP_P && which != MG_OP_R) return fail(MG_ERR_INVALID, "bad operator selector %lld", which);
  if (which != MG_OP_A && level == h->nlevels) return fail(MG_ERR_INVALID, "the coarsest level %lld has no transfer operators", level);
  (void)hipSetDevice(h->device);
  CxLevel& L = h->cx->lev[(size_t)level - 1];
  MG_TRY(cx_upload(which == MG_OP_A ? &L.A : which == MG_OP_P ? &L.P : &L.R, h->opt, n_rows, n_cols, colptr, rowval, nzval, which == MG_OP_A));
  h->cx->finalized = false;
  return MG_OK;
}

int mg_set_relax_CF32(mg_hierarchy* h, long long level, const float* d, long long n, long long relaxPre, long long relaxPost) {
  UploadFence upload_fence;
  MG_TRY(cx_level_ok(h, level, CX_WANT32));
  if (!d || n < 1) return fail(MG_ERR_INVALID, "empty relaxPrec");
  if (relaxPre < 0 || relaxPost < 0) return fail(MG_ERR_INVALID, "negative sweep count");
  (void)hipSetDevice(h->device);
  CxLevel& L = h->cx->lev[(size_t)level - 1];
  MG_TRY(L.d.alloc((size_t)n));   // n float pairs
  HIP_TRY(hipMemcpy(L.d.p, d, 2 * (size_t)n * sizeof(float), hipMemcpyHostToDevice));
  L.relax_set = true;
  L.npre = relaxPre;
  L.npost = relaxPost;
  h->cx->finalized = false;
  return MG_OK;
}

int mg_set_coarse_dense_inverse_CF64(mg_hierarchy* h, long long n, const double* Ainv) {
  UploadFence upload_fence;
  MG_TRY(cx_level_ok(h, 1, CX_ANY));   // (a CF32 handle's coarsest solve stays ComplexF64)
  if (n < 1 || !Ainv) return fail(MG_ERR_INVALID, "empty coarse inverse");
  if (n > 32000) return fail(MG_ERR_UNSUPPORTED, "dense coarse inverse of order %lld is too large", n);
  (void)hipSetDevice(h->device);
  CxState& S = *h->cx;
  std::vector<double> rm(2 * (size_t)n * (size_t)n);   // column-major -> row-major, (re, im) pairs
  for (long long j = 0; j < n; ++j)
    for (long long i = 0; i < n; ++i) {
      rm[2 * ((size_t)i * n + j)] = Ainv[2 * ((size_t)j * n + i)];
      rm[2 * ((size_t)i * n + j) + 1] = Ainv[2 * ((size_t)j * n + i) + 1];
    }
  MG_TRY(S.Ainv.alloc(rm.size()));
  HIP_TRY(hipMemcpy(S.Ainv.p, rm.data(), rm.size() * sizeof(double), hipMemcpyHostToDevice));
  dd_detach(h);
  cx_drop_coarse_appliers(S);
  S.n_coarse = n;
  S.coarse_set = true;
  S.coarse_lu = false;
  S.coarse_gmres = false;
  S.finalized = false;
  return MG_OK;
}

// The explicit inverse of the resident coarsest operator, built in HBM (mg_dense_inv.hpp) - the device twin of the setter above.
// cx_coarse_inverse_check: what is refused before the first write; cx_coarse_inverse_enqueue: the launches on the handle's stream
// into `spare`; cx_coarse_inverse_finish (behind the caller's synchronisation): the flag read, `spare` exchanged with Ainv when clean.
static int cx_coarse_inverse_check(mg_hierarchy* h) {
  CxState& S = *h->cx;
  const CxMat& A = S.lev[(size_t)h->nlevels - 1].A;
  if (!A.set) return fail(MG_ERR_STATE, "the coarsest operator was not uploaded");
  if (A.wide) return fail(MG_ERR_UNSUPPORTED, "the coarsest operator holds 64-bit row pointers: the device inverse serves int32 operators");
  if (A.n_rows != A.n_cols) return fail(MG_ERR_INVALID, "the coarsest operator is %lld x %lld", A.n_rows, A.n_cols);
  if (A.n_rows > dense_inv_max(h->opt))
    return fail(MG_ERR_UNSUPPORTED, "the coarsest operator has %lld rows: the device inverse serves up to %lld (option coarse_device_inverse_max)",
                A.n_rows, dense_inv_max(h->opt));
  return MG_OK;
}
static int cx_coarse_inverse_enqueue(mg_hierarchy* h, DenseInv<cx_t>& K, DevBuf<double>& spare) {
  const CxMat& A = h->cx->lev[(size_t)h->nlevels - 1].A;
  const hipStream_t st = h->play->stream;
  if (A.single)   // (a CF32 handle's coarsest operator, widened as the host does with astype(complex128))
    return coarse_inverse_enqueue<cx_t, cf_t>(K, spare, A.n_rows, A.rowptr.p, A.colidx.p, reinterpret_cast<const cf_t*>(A.valf.p), st);
  return coarse_inverse_enqueue<cx_t, cx_t>(K, spare, A.n_rows, A.rowptr.p, A.colidx.p, reinterpret_cast<const cx_t*>(A.val.p), st);
}
static int cx_coarse_inverse_finish(mg_hierarchy* h, DenseInv<cx_t>& K, DevBuf<double>& spare, const char* who) {
  int col = 0;
  const int rc = K.singular_column(&col);
  if (rc != MG_OK || col != 0) {
    spare.release();
    return rc != MG_OK ? rc
                       : fail(MG_ERR_INVALID, "%s: the coarsest operator is singular to working precision (zero or non-finite pivot in column %d): the previous inverse stays",
                              who, col);
  }
  std::swap(h->cx->Ainv, spare);
  spare.release();
  return MG_OK;
}

int mg_build_coarse_dense_inverse_CF64(mg_hierarchy* h) {
  MG_TRY(cx_level_ok(h, 1, CX_ANY));   // (a CF32 handle's coarsest solve stays ComplexF64)
  MG_TRY(cx_coarse_inverse_check(h));
  (void)hipSetDevice(h->device);
  CxState& S = *h->cx;
  DenseInv<cx_t> K;
  DevBuf<double> spare;
  int rc = cx_coarse_inverse_enqueue(h, K, spare);
  if (spin_sync(h->play->stream) != hipSuccess && rc == MG_OK) rc = fail(MG_ERR_HIP, "mg_build_coarse_dense_inverse_CF64: stream failed");
  if (rc != MG_OK) {
    spare.release();
    return rc;
  }
  MG_TRY(cx_coarse_inverse_finish(h, K, spare, "mg_build_coarse_dense_inverse_CF64"));
  dd_detach(h);
  cx_drop_coarse_appliers(S);
  for (DevBuf<int>* q : {&S.luLptr, &S.luLcol, &S.luUptr, &S.luUcol, &S.luP, &S.luQ, &S.luLorder, &S.luLlvl, &S.luUorder, &S.luUlvl}) q->release();
  S.luLval.release(); S.luUval.release(); S.luWork.release();
  S.n_coarse = S.lev[(size_t)h->nlevels - 1].A.n_rows;
  S.coarse_set = true;
  S.coarse_lu = false;
  S.coarse_gmres = false;
  S.finalized = false;
  return MG_OK;
}

int mg_get_coarse_dense_inverse_CF64(mg_hierarchy* h, long long n, double* out) {
  MG_TRY(cx_level_ok(h, 1, CX_ANY));
  if (!out) return fail(MG_ERR_INVALID, "null argument");
  CxState& S = *h->cx;
  if (!S.coarse_set || S.coarse_lu || S.coarse_gmres || h->coarse_dd || !S.Ainv.p)
    return fail(MG_ERR_STATE, "the coarsest solve of this handle is not a dense inverse");
  if (n != S.n_coarse) return fail(MG_ERR_INVALID, "n=%lld differs from the coarsest order %lld", n, S.n_coarse);
  (void)hipSetDevice(h->device);
  HIP_TRY(spin_sync(h->play->stream));
  return dense_inverse_readback<2>(S.Ainv, n, out);
}

int mg_dense_inverse_CF64(long long device, long long n, const double* A, double* out) {
  MG_TRY(dense_inverse_args(n, A, out, "mg_dense_inverse_CF64"));
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(MG_ERR_INVALID, "device=%lld but %d devices visible", device, ndev);
  HIP_TRY(hipSetDevice((int)device));
  return dense_inverse_host<cx_t>(n, A, out, "mg_dense_inverse_CF64");
}

int mg_set_coarse_lu_CF64_INT64(mg_hierarchy* h, long long n, const long long* Lptr, const long long* Lcol, const double* Lval,
                                const long long* Uptr, const long long* Ucol, const double* Uval, const long long* p,
                                const long long* q) {
  UploadFence upload_fence;
  MG_TRY(cx_level_ok(h, 1, CX_ANY));
  if (n < 1 || !Lptr || !Lcol || !Lval || !Uptr || !Ucol || !Uval || !p || !q) return fail(MG_ERR_INVALID, "null or empty factor");
  if (n >= (1LL << 31) - 1 || Lptr[n] - 1 >= (1LL << 31) || Uptr[n] - 1 >= (1LL << 31))
    return fail(MG_ERR_UNSUPPORTED, "factors exceed int32 device indices");
  if (Lptr[0] != 1 || Uptr[0] != 1) return fail(MG_ERR_INVALID, "row pointers must be 1-based");
  (void)hipSetDevice(h->device);
  CxState& S = *h->cx;
  if (h->play->stream) HIP_TRY(spin_sync(h->play->stream));
  if (n >= h->opt.lu_multi_min_rows) {
    // the chip-wide form, as the real hierarchy selects it (mg_set_coarse_lu_FP64_INT64): per-level launches and a dense trailing
    // inverse, held by a factor applier of the hierarchy's own and enqueued on the hierarchy's stream (cx_coarse)
    CxLu* F = nullptr;
    MG_TRY(cxlu_create(h->device, n, Lptr, Lcol, Lval, Uptr, Ucol, Uval, p, q, &F, &h->opt));
    const size_t wlen = (size_t)n, tlen = (size_t)std::max(F->fwd->M, 1);   // (no allocation inside the cycle)
    if (F->work.alloc(wlen) != MG_OK || F->tail.alloc(tlen) != MG_OK) {
      cxlu_destroy(F);
      return fail(MG_ERR_HIP, "allocation of the coarsest solve's work vectors failed");
    }
    cx_drop_coarse_appliers(S);
    S.coarse_multi = F;
    for (DevBuf<int>* d : {&S.luLptr, &S.luLcol, &S.luUptr, &S.luUcol, &S.luP, &S.luQ, &S.luLorder, &S.luLlvl, &S.luUorder, &S.luUlvl}) d->release();
    S.luLval.release(); S.luUval.release(); S.luWork.release();
    dd_detach(h);
    S.n_coarse = n;
    S.coarse_set = true;
    S.coarse_lu = true;
    S.coarse_gmres = false;
    S.Ainv.release();
    S.finalized = false;
    return MG_OK;
  }
  cx_drop_coarse_appliers(S);
  const size_t N = (size_t)n;
  std::vector<int> LP, LC, LO, LL, UP, UC, UO, UL, pp(N), qq(N);
  MG_TRY(lu_convert(n, Lptr, Lcol, true, LP, LC, LO, LL));
  MG_TRY(lu_convert(n, Uptr, Ucol, false, UP, UC, UO, UL));
  for (size_t i = 0; i < N; ++i) {
    if (p[i] < 1 || p[i] > n || q[i] < 1 || q[i] > n) return fail(MG_ERR_INVALID, "permutation entry out of range");
    pp[i] = (int)(p[i] - 1);
    qq[i] = (int)(q[i] - 1);
  }
  auto up_i = [&](DevBuf<int>& d, const std::vector<int>& v) -> int {
    MG_TRY(d.alloc(v.size()));
    HIP_TRY(hipMemcpy(d.p, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
    return MG_OK;
  };
  MG_TRY(up_i(S.luLptr, LP)); MG_TRY(up_i(S.luLcol, LC)); MG_TRY(up_i(S.luLorder, LO)); MG_TRY(up_i(S.luLlvl, LL));
  MG_TRY(up_i(S.luUptr, UP)); MG_TRY(up_i(S.luUcol, UC)); MG_TRY(up_i(S.luUorder, UO)); MG_TRY(up_i(S.luUlvl, UL));
  MG_TRY(up_i(S.luP, pp)); MG_TRY(up_i(S.luQ, qq));
  MG_TRY(S.luLval.alloc(2 * LC.size()));
  MG_TRY(S.luUval.alloc(2 * UC.size()));
  HIP_TRY(hipMemcpy(S.luLval.p, Lval, 2 * LC.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(S.luUval.p, Uval, 2 * UC.size() * sizeof(double), hipMemcpyHostToDevice));
  S.nLlvl = (int)LL.size() - 1;
  S.nUlvl = (int)UL.size() - 1;
  dd_detach(h);
  S.n_coarse = n;
  S.coarse_set = true;
  S.coarse_lu = true;
  S.coarse_gmres = false;
  S.Ainv.release();
  S.finalized = false;
  return MG_OK;
}

// ComplexF32 factors on a CF32 handle (the reference's parallelJuliaSolver(ComplexF32, Int64) as param.LU): the coarsest solve applies
// them to the cycle's own float2 bc - no widened pair - in the single-workgroup form below lu_multi_min_rows rows and the chip-wide
// form from there on, both held by a factor applier of the hierarchy's own and enqueued on the hierarchy's stream (cx_coarse).
int mg_set_coarse_lu_CF32_INT64(mg_hierarchy* h, long long n, const long long* Lptr, const long long* Lcol, const float* Lval,
                                const long long* Uptr, const long long* Ucol, const float* Uval, const long long* p,
                                const long long* q) {
  UploadFence upload_fence;
  MG_TRY(cx_level_ok(h, 1, CX_WANT32));
  if (n < 1 || !Lptr || !Lcol || !Lval || !Uptr || !Ucol || !Uval || !p || !q) return fail(MG_ERR_INVALID, "null or empty factor");
  if (n >= (1LL << 31) - 1 || Lptr[n] - 1 >= (1LL << 31) || Uptr[n] - 1 >= (1LL << 31))
    return fail(MG_ERR_UNSUPPORTED, "factors exceed int32 device indices");
  if (Lptr[0] != 1 || Uptr[0] != 1) return fail(MG_ERR_INVALID, "row pointers must be 1-based");
  (void)hipSetDevice(h->device);
  CxState& S = *h->cx;
  if (h->play->stream) HIP_TRY(spin_sync(h->play->stream));
  CxLuT<cf_t>* F = nullptr;
  MG_TRY(cxlu_create<cf_t>(h->device, n, Lptr, Lcol, Lval, Uptr, Ucol, Uval, p, q, &F, &h->opt));
  const size_t wlen = (size_t)n, tlen = (size_t)std::max(F->fwd->M, 1);   // (no allocation inside the cycle)
  if (F->work.alloc(wlen) != MG_OK || F->tail.alloc(tlen) != MG_OK) {
    cxlu_destroy(F);
    return fail(MG_ERR_HIP, "allocation of the coarsest solve's work vectors failed");
  }
  cx_drop_coarse_appliers(S);
  S.coarse_single = F;
  for (DevBuf<int>* d : {&S.luLptr, &S.luLcol, &S.luUptr, &S.luUcol, &S.luP, &S.luQ, &S.luLorder, &S.luLlvl, &S.luUorder, &S.luUlvl}) d->release();
  S.luLval.release(); S.luUval.release(); S.luWork.release();
  dd_detach(h);
  S.n_coarse = n;
  S.coarse_set = true;
  S.coarse_lu = true;
  S.coarse_gmres = false;
  S.Ainv.release();
  S.finalized = false;
  return MG_OK;
}

// coarseSolveType "GMRES": d = param.LU = relaxParam ./ diag(A_c), n complex128 values (a CF32 handle's too)
int mg_set_coarse_gmres_CF64(mg_hierarchy* h, long long n, const double* d) {
  UploadFence upload_fence;
  MG_TRY(cx_level_ok(h, 1, CX_ANY));
  if (n < 1 || !d) return fail(MG_ERR_INVALID, "empty coarsest Jacobi vector");
  if (n >= (1LL << 31) - 1) return fail(MG_ERR_UNSUPPORTED, "dimension exceeds int32 device indices");
  (void)hipSetDevice(h->device);
  CxState& S = *h->cx;
  if (h->play->stream) HIP_TRY(spin_sync(h->play->stream));
  MG_TRY(S.cgD.alloc(2 * (size_t)n));
  HIP_TRY(hipMemcpy(S.cgD.p, d, 2 * (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  dd_detach(h);
  cx_drop_coarse_appliers(S);
  for (DevBuf<int>* q : {&S.luLptr, &S.luLcol, &S.luUptr, &S.luUcol, &S.luP, &S.luQ, &S.luLorder, &S.luLlvl, &S.luUorder, &S.luUlvl}) q->release();
  S.luLval.release(); S.luUval.release(); S.luWork.release();
  S.Ainv.release();
  S.n_coarse = n;
  S.coarse_set = true;
  S.coarse_lu = false;
  S.coarse_gmres = true;
  S.finalized = false;
  return MG_OK;
}

// The GMRES coarsest solve alone on host arrays, behind the entry points' checks: b staged (W: a vector, or a column-major block relaid),
// the vector or the block solve, x back, the report copied out.  (The staging blocks of the block work set are sized by the FINE level.)
static int cx_coarse_gmres_host(mg_hierarchy* h, const double* b, double* x, long long n, CxCols W, long long* steps, long long* flag,
                                double* resvec) {
  (void)hipSetDevice(h->device);
  MG_TRY(W.ensure(h));
  CxCoarseReport report;
  DevBuf<double> cm, db, dx;   // (released below on every path)
  int rc = W.nr ? cm.alloc(2 * W.len(n)) : MG_OK;
  if (rc == MG_OK) rc = db.alloc(2 * W.len(n));
  if (rc == MG_OK) rc = dx.alloc(2 * W.len(n));
  if (rc == MG_OK) rc = W.upload(h, b, cm, cxp(db), n);
  if (rc == MG_OK) rc = W.nr ? cx_coarse_block_gmres(h, cxc(db), cxp(dx), W.nr, &report) : cx_coarse_gmres(h, cxc(db), cxp(dx), &report);
  if (rc == MG_OK) rc = W.download(h, cxc(dx), cm, x, n);
  if (spin_sync(h->play->stream) != hipSuccess && rc == MG_OK) rc = fail(MG_ERR_HIP, "mg_coarse_gmres_CF64: stream failed");
  cm.release();
  db.release();
  dx.release();
  if (rc != MG_OK) return rc;
  if (steps) *steps = report.used;
  if (flag) *flag = report.flag;
  if (resvec)
    for (int i = 0; i < report.used; ++i) resvec[i] = report.resvec[i];
  return MG_OK;
}

// the coarsest solve alone on host vectors: x = the GMRES coarsest solve of b; steps = the columns used, flag 0 / -1 / -9,
// resvec[i] = err_i / ||b|| for i < steps (10 entries at most)
int mg_coarse_gmres_CF64(mg_hierarchy* h, const double* b, double* x, long long n, long long* steps, long long* flag, double* resvec) {
  MG_TRY(cx_level_ok(h, 1, CX_ANY));
  CxState& S = *h->cx;
  if (!S.finalized) return fail(MG_ERR_STATE, "hierarchy not finalized: call mg_finalize first");
  if (!S.coarse_gmres) return fail(MG_ERR_STATE, "the coarsest solve of this handle is not GMRES (mg_set_coarse_gmres_CF64)");
  if (!b || !x) return fail(MG_ERR_INVALID, "null vector");
  if (n != S.n_coarse) return fail(MG_ERR_INVALID, "n=%lld does not match the coarsest level (%lld rows)", n, S.n_coarse);
  return cx_coarse_gmres_host(h, b, x, n, CxCols::vec(), steps, flag, resvec);
}

// The block form of the solve alone on host blocks (option coarse_gmres_blocks): b, x column-major n x nrhs, n = the coarsest order;
// steps, flag and resvec (10 entries at most: ||xi - H Y||_F / ||B||_F per step) are those of the whole block.  nrhs = 1 is the
// single-vector solve.
int mg_block_coarse_gmres_CF64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs, long long* steps, long long* flag,
                               double* resvec) {
  MG_TRY(cx_level_ok(h, 1, CX_ANY));
  CxState& S = *h->cx;
  if (!S.finalized) return fail(MG_ERR_STATE, "hierarchy not finalized: call mg_finalize first");
  if (!S.coarse_gmres) return fail(MG_ERR_STATE, "the coarsest solve of this handle is not GMRES (mg_set_coarse_gmres_CF64)");
  MG_TRY(cx_block_nrhs_ok(nrhs));
  MG_TRY(cx_block_coarse_ok(h, nrhs));
  if (!b || !x) return fail(MG_ERR_INVALID, "null block");
  if (n != S.n_coarse) return fail(MG_ERR_INVALID, "n=%lld does not match the coarsest level (%lld rows)", n, S.n_coarse);
  return cx_coarse_gmres_host(h, b, x, n, nrhs == 1 ? CxCols::vec() : CxCols::blk(nrhs), steps, flag, resvec);
}

// info[0]: 1 where blocks are served on this handle's GMRES coarsest solve (option coarse_gmres_blocks), 0 otherwise; info[1]: kernel
// launches of one block solve of nrhs columns on the path in use (the chain: front 3, step j: j + 5, the combination; the one-workgroup
// form: front 1, 2 per step, the combination); info[2]: that path (0: the chain of grid-wide passes, 1: the one-workgroup form)
int mg_block_coarse_form(mg_hierarchy* h, long long nrhs, long long* info) {
  if (!h || !info) return fail(MG_ERR_INVALID, "null argument");
  if (!h->cx || !h->cx->coarse_set) return fail(MG_ERR_STATE, "the coarsest solve of a complex handle was not set");
  MG_TRY(cx_block_nrhs_ok(nrhs));
  const bool on = h->cx->coarse_gmres && h->opt.coarse_gmres_blocks && !h->coarse_dd;
  info[0] = on ? 1 : 0;
  info[1] = !on ? 0 : nrhs == 1 ? cx_cg_launches(h) : cx_cb_launches(h, (int)nrhs);
  info[2] = !on ? 0 : nrhs == 1 ? (cx_cg_use_tail(h) ? 1 : 0) : (cx_cb_use_tail(h, (int)nrhs) ? 1 : 0);
  return MG_OK;
}

int mg_cycle_CF64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs, long long x_is_zero) {
  return cx_cycle_host<cx_t>(h, b, x, n, x_is_zero, CX_WANT64, CxCols::vec(nrhs));
}
int mg_cycle_CF32(mg_hierarchy* h, const float* b, float* x, long long n, long long nrhs, long long x_is_zero) {
  return cx_cycle_host<cf_t>(h, b, x, n, x_is_zero, CX_WANT32, CxCols::vec(nrhs));
}

int mg_solve_CF64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs, double tol, long long maxIter,
                  long long* iters, double* resvec) {
  return cx_solve_host<cx_t>(h, b, x, n, tol, maxIter, iters, resvec, CX_WANT64, CxCols::vec(nrhs));
}
int mg_solve_CF32(mg_hierarchy* h, const float* b, float* x, long long n, long long nrhs, double tol, long long maxIter,
                  long long* iters, double* resvec) {
  return cx_solve_host<cf_t>(h, b, x, n, tol, maxIter, iters, resvec, CX_WANT32, CxCols::vec(nrhs));
}

int mg_spmv_CF64(mg_hierarchy* h, long long level, long long which, const double* alpha, const double* x, const double* beta,
                 double* y, long long nrhs) {
  return cx_spmv_host<cx_t>(h, level, which, alpha, x, beta, y, CX_WANT64, CxCols::vec(nrhs));
}
int mg_spmv_CF32(mg_hierarchy* h, long long level, long long which, const float* alpha, const float* x, const float* beta, float* y,
                 long long nrhs) {
  return cx_spmv_host<cf_t>(h, level, which, alpha, x, beta, y, CX_WANT32, CxCols::vec(nrhs));
}

// blocks of right-hand sides on a CF64 handle: nrhs arrives with each call (the device-pointer forms and the block driver, which
// also serve CF32 handles, are in mg_complex_krylov.inc)
int mg_block_spmv_CF64(mg_hierarchy* h, long long level, long long which, const double* alpha, const double* X, const double* beta,
                       double* Y, long long nrhs) {
  return cx_spmv_host<cx_t>(h, level, which, alpha, X, beta, Y, CX_WANT64, CxCols::blk(nrhs));
}
int mg_block_cycle_CF64(mg_hierarchy* h, const double* B, double* X, long long n, long long nrhs, long long x_is_zero) {
  return cx_cycle_host<cx_t>(h, B, X, n, x_is_zero, CX_WANT64, CxCols::blk(nrhs));
}
int mg_block_solve_CF64(mg_hierarchy* h, const double* B, double* X, long long n, long long nrhs, double tol, long long maxIter,
                        long long* iters, double* resvec) {
  return cx_solve_host<cx_t>(h, B, X, n, tol, maxIter, iters, resvec, CX_WANT64, CxCols::blk(nrhs));
}

}  // extern "C"

namespace {

// replaceMatrixInHierarchy on the device (MGsetup.jl:226-270) for VAL = ComplexF64 or ComplexF32 (C: the handle's pair type, cx_t or
// cf_t): new fine values on the stored pattern, then per level relaxPrecs[l] = getRelaxPrec(As[l]) and As[l+1] = Rs[l]*(As[l]*Ps[l]) on
// the fixed patterns.  Generic CSR has no derived formats to rebuild.  A CF32 handle's kernels read the single values, compute in
// ComplexF64 and round once on the store (mg_complex.hpp).  The coarsest solve: with the option coarse_device_inverse and a dense
// inverse installed, the inverse of the new coarsest operator is built in HBM behind the last Galerkin product (mg_dense_inv.hpp), on
// the same stream and inside the call's one synchronisation - a singular operator is an error return and the previous inverse stays;
// the GMRES coarsest solve recomputes its Jacobi vector there (a CF32 handle: from the coarsest operator widened again into cgA, ahead
// of it).  Otherwise the factorisation stays with the host: mg_get_values_* of the coarsest level, factor,
// mg_set_coarse_dense_inverse_CF64 / mg_set_coarse_lu_CF64_INT64, mg_finalize.  A CF32 handle's auto-widened Krylov operator is
// dropped: the next driver call widens the new As[1].  The checks of arguments and state precede the first write.
template <typename C>
int cx_rap(mg_hierarchy* h, const typename mgk::cx_scalar<C>::type* fine_nzval, long long nnz, long long relaxKind, const double* omega,
           long long* levels_done, const char* who, const char* sfx) {
  typedef typename mgk::cx_scalar<C>::type ST;
  CxState& S = *h->cx;
  if (!S.finalized) return fail(MG_ERR_STATE, "hierarchy not finalized: call mg_finalize first");
  if (nnz != S.lev[0].A.nnz) return fail(MG_ERR_INVALID, "nnz=%lld differs from the stored fine pattern (%lld)", nnz, S.lev[0].A.nnz);
  if (relaxKind != 0 && relaxKind != 1) return fail(MG_ERR_INVALID, "relaxKind must be 0 (Jac) or 1 (SPAI)");
  const bool vanka = h->relax_type == 2;
  if (vanka && !h->opt.vanka_device_setup)
    return fail(MG_ERR_UNSUPPORTED, "%s recomputes Jac and SPAI relaxPrecs: the blocks of a Vanka handle are set up on the host", who);
  const int nl = (int)h->nlevels;
  if (vanka)   // option vanka_device_setup: every relaxed level's blocks are built again with what mg_build_vanka_* was given
    for (int l = 0; l + 1 < nl; ++l) {
      const CxLevel& L = S.lev[(size_t)l];
      if (!L.vanka || !L.vanka->has_w)
        return fail(MG_ERR_STATE, "level %d's Vanka blocks were bound by mg_set_vanka_%s: no (VankaType, w) to build them again with (mg_build_vanka_%s)", l + 1,
                    sfx, sfx);
    }
  for (int l = 0; l < nl; ++l) {
    const CxLevel& L = S.lev[(size_t)l];
    if (L.A.wide || (l + 1 < nl && (L.P.wide || L.R.wide)))
      return fail(MG_ERR_UNSUPPORTED, "level %d holds an operator with 64-bit row pointers: the numeric Galerkin product on the device serves int32 operators", l + 1);
  }
  for (int l = 1; l < nl; ++l)
    if (!S.lev[(size_t)l].A.rows_sorted)
      return fail(MG_ERR_UNSUPPORTED, "As[%d] holds a row whose stored columns do not ascend: the numeric Galerkin product on the device finds its target columns by binary search (sort the rows, or take the host path)", l + 1);
  const bool dev_inverse = h->opt.coarse_device_inverse && S.coarse_set && !S.coarse_lu && !S.coarse_gmres && !h->coarse_dd && S.Ainv.p;
  if (dev_inverse) MG_TRY(cx_coarse_inverse_check(h));
  if (S.single && S.coarse_gmres && (!S.cgA.set || S.cgA.nnz != S.lev[(size_t)nl - 1].A.nnz))
    return fail(MG_ERR_STATE, "the widened coarsest operator of the GMRES coarsest solve is missing: call mg_finalize first");
  (void)hipSetDevice(h->device);
  const hipStream_t st = h->play->stream;
  if (relaxKind == 1)
    for (int l = 0; l + 1 < nl; ++l) MG_TRY(cx_build_transposed_pattern(S.lev[(size_t)l].A));   // (first SPAI re-setup only)
  while (S.rap_ev.size() < (size_t)nl) {
    hipEvent_t e;
    HIP_TRY(hipEventCreate(&e));
    S.rap_ev.push_back(e);
  }
  S.rap_timed = false;
  MG_TRY(cx_write_values<ST>(h, S.lev[0].A, fine_nzval));
  for (int l = 0; l + 1 < nl; ++l) {
    CxLevel& L = S.lev[(size_t)l];
    CxMat& Cm = S.lev[(size_t)l + 1].A;
    const unsigned nb = cx_grid(L.n);
    const mgk::CxCsr32<C> Ad = cx_csr32<C>(L.A);
    HIP_TRY(hipEventRecord(S.rap_ev[(size_t)l], st));
    if (vanka) {   // the level's blocks from its new values, into the spare buffer (exchanged below, once nothing was found singular)
      MG_TRY(vanka_build_launch(L.vanka, L.A.rowptr.p, L.A.colidx.p, L.A.vals(), L.vanka->built, st));
    } else if (relaxKind == 0) {
      hipLaunchKernelGGL((mgk::cx_relax_jacobi<C, C>), dim3(nb), dim3(mgk::BLK), 0, st, Ad, (int)L.n, omega[l], cxp<C>(L.d));
    } else {   // the level's r as scratch for the column sums (one double per row in either precision)
      hipLaunchKernelGGL((mgk::cx_colsumsq<C>), dim3(nb), dim3(mgk::BLK), 0, st, static_cast<const C*>(L.A.vals()), L.A.t_ptr.p,
                         L.A.t_perm.p, (int)L.A.n_cols, L.r.p);
      hipLaunchKernelGGL((mgk::cx_relax_spai<C>), dim3(nb), dim3(mgk::BLK), 0, st, Ad, (int)L.n, omega[l], L.r.p, cxp<C>(L.d));
    }
    const long long cap = std::max<long long>(1, std::min<long long>(h->opt.rap_chunk, mgk::RAP_CAP));
    const int chunk = (int)std::max<long long>(1, std::min<long long>(cap, Cm.max_row));
    // lane groups: the default (option rap_groups: 1, 2, 4, 8, 16), halved while the accumulator copies exceed 32 KB of LDS
    // (the accumulator holds ComplexF64 sums in either precision)
    int groups = 1;
    while (groups * 2 <= std::min<long long>(h->opt.rap_groups > 0 ? h->opt.rap_groups : mgk::CX_RAP_GROUPS, 16)) groups *= 2;
    while (groups > 1 && (size_t)chunk * ((size_t)groups * sizeof(cx_t) + sizeof(int)) > 32768) groups /= 2;
    hipLaunchKernelGGL((mgk::cx_rap_numeric<C, ST>), dim3((unsigned)Cm.n_rows), dim3(64), (size_t)chunk * ((size_t)groups * sizeof(cx_t) + sizeof(int)), st,
                       cx_csr32<ST>(L.R), Ad, cx_csr32<ST>(L.P), Cm.rowptr.p, Cm.colidx.p, static_cast<C*>(const_cast<void*>(Cm.vals())), chunk, groups);
    HIP_TRY(hipGetLastError());
  }
  if (S.coarse_gmres) {   // param.LU = relaxParam ./ diag(A_c) on the new coarsest operator (MGsetup.jl:335-336): omega[nlevels - 1]
    const CxLevel& Lc = S.lev[(size_t)nl - 1];
    if (S.single) MG_TRY(cx_widen_values(h, Lc.A, S.cgA));   // (the operator the coarsest solve applies: ahead of everything that reads it)
    hipLaunchKernelGGL((mgk::cx_relax_jacobi<cx_t, cx_t>), dim3(cx_grid(Lc.n)), dim3(mgk::BLK), 0, st, cx_csr32<cx_t>(cx_cg_operator(S)), (int)Lc.n,
                       omega[nl - 1], cxp(S.cgD));
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(S.rap_ev[(size_t)nl - 1], st));
  DenseInv<cx_t> inv;        // option coarse_device_inverse: the new coarsest operator's inverse, into a spare buffer (exchanged below)
  DevBuf<double> inv_spare;
  int inv_rc = dev_inverse ? cx_coarse_inverse_enqueue(h, inv, inv_spare) : MG_OK;
  const hipError_t synced = spin_sync(st);
  if (synced != hipSuccess || inv_rc != MG_OK) {
    inv_spare.release();
    if (inv_rc != MG_OK) return inv_rc;
    HIP_TRY(synced);
  }
  S.rap_timed = true;
  if (S.single && S.K_auto) {   // As[1] widened for the Krylov drivers holds the old values: the next driver call widens the new ones
    S.K.release();
    S.K_auto = false;
  }
  if (dev_inverse) inv_rc = cx_coarse_inverse_finish(h, inv, inv_spare, who);
  if (vanka) {   // a singular cell anywhere: no level's blocks are exchanged (the operators hold the new values; the blocks the old ones)
    int bad = 0, first = 0;
    for (int l = 0; l + 1 < nl; ++l) {
      VankaCore* V = S.lev[(size_t)l].vanka;
      int flag[2] = {0, 0};
      HIP_TRY(hipMemcpy(flag, V->flag.p, sizeof(flag), hipMemcpyDeviceToHost));
      if (flag[0] != 0)
        return fail(MG_ERR_INVALID, "%s: level %d: cell %d of %d with a singular block: every level keeps its previous blocks", who, l + 1,
                    INT_MAX - flag[1] + 1, flag[0]);
    }
    for (int l = 0; l + 1 < nl; ++l) {
      VankaCore* V = S.lev[(size_t)l].vanka;
      MG_TRY(vanka_build_finish(V, V->built, &bad, &first));
    }
  }
  if (levels_done) *levels_done = nl - 1;
  return inv_rc;   // (a singular coarsest operator: the operators hold the new values, the coarsest solve the previous inverse)
}

// Device time of the last mg_rap_* of the handle, level by level (relaxPrecs[l] and As[l+1] together), in milliseconds
int cx_rap_level_ms(mg_hierarchy* h, double* out, long long n, const char* rap) {
  CxState& S = *h->cx;
  if (!out || n != h->nlevels - 1) return fail(MG_ERR_INVALID, "out must hold nlevels - 1 = %lld values", h->nlevels - 1);
  if (!S.rap_timed) return fail(MG_ERR_STATE, "no completed %s on this handle", rap);
  for (long long l = 0; l < n; ++l) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, S.rap_ev[(size_t)l], S.rap_ev[(size_t)l + 1]));
    out[l] = (double)ms;
  }
  return MG_OK;
}

// mg_get_values_* / mg_get_relax_* / mg_replace_values_* behind the handle checks of their entry points; ST: the host scalar of the
// handle's precision.  Complex values leave and arrive in the reference's AT convention.
template <typename ST>
int cx_get_values(mg_hierarchy* h, long long level, long long which, ST* out, long long nnz, CxWant want) {
  CxMat* M;
  MG_TRY(cx_find_op(h, level, which, &M, want));
  if (nnz != M->nnz) return fail(MG_ERR_INVALID, "nnz=%lld differs from the stored pattern (%lld)", nnz, M->nnz);
  (void)hipSetDevice(h->device);
  HIP_TRY(spin_sync(h->play->stream));
  const size_t len = (size_t)nnz * (M->cplx ? 2 : 1);
  if (len > 0) HIP_TRY(hipMemcpy(out, M->vals(), len * sizeof(ST), hipMemcpyDeviceToHost));
  if (M->cplx)   // back to the reference's AT convention
    for (size_t k = 1; k < len; k += 2) out[k] = -out[k];
  return MG_OK;
}

template <typename ST>
int cx_get_relax(mg_hierarchy* h, long long level, ST* out, long long n, CxWant want) {
  MG_TRY(cx_level_ok(h, level, want));
  CxLevel& L = h->cx->lev[(size_t)level - 1];
  if (!L.relax_set || (long long)cx_len(*h->cx, n) != (long long)L.d.n) return fail(MG_ERR_INVALID, "relaxPrecs[%lld] not set or wrong length", level);
  (void)hipSetDevice(h->device);
  HIP_TRY(spin_sync(h->play->stream));
  HIP_TRY(hipMemcpy(out, L.d.p, 2 * (size_t)n * sizeof(ST), hipMemcpyDeviceToHost));
  return MG_OK;
}

template <typename ST>
int cx_replace_values(mg_hierarchy* h, long long level, long long which, const ST* nzval, long long nnz, CxWant want) {
  CxMat* M;
  MG_TRY(cx_find_op(h, level, which, &M, want));
  if (nnz != M->nnz) return fail(MG_ERR_INVALID, "nnz=%lld differs from the stored pattern (%lld)", nnz, M->nnz);
  (void)hipSetDevice(h->device);
  return cx_write_values<ST>(h, *M, nzval);
}

}  // namespace

extern "C" {

int mg_rap_CF64(mg_hierarchy* h, const double* fine_nzval, long long nnz, long long relaxKind, const double* omega,
                long long* levels_done) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  if (!fine_nzval || !omega) return fail(MG_ERR_INVALID, "null argument");
  if (!h->cx) return fail(MG_ERR_STATE, "CF64 entry point called on an FP64 handle (create it with mg_create_CF64)");
  MG_CF32_UNSUPPORTED(h);   // (its _CF32 twin serves a CF32 hierarchy)
  return cx_rap<cx_t>(h, fine_nzval, nnz, relaxKind, omega, levels_done, "mg_rap_CF64", "CF64");
}

// The same for a CF32 handle: fine values, As and relaxPrecs in single, every sum in ComplexF64, one rounding on the store.
int mg_rap_CF32(mg_hierarchy* h, const float* fine_nzval, long long nnz, long long relaxKind, const double* omega,
                long long* levels_done) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  if (!fine_nzval || !omega) return fail(MG_ERR_INVALID, "null argument");
  MG_TRY(cx_handle_ok(h, CX_WANT32));
  return cx_rap<cf_t>(h, fine_nzval, nnz, relaxKind, omega, levels_done, "mg_rap_CF32", "CF32");
}

// Device time of the last mg_rap_CF64, level by level (relaxPrecs[l] and As[l+1] together), in milliseconds: out[0 .. nlevels-1).
int mg_rap_level_ms_CF64(mg_hierarchy* h, double* out, long long n) {
  MG_CF32_UNSUPPORTED(h);
  MG_TRY(cx_level_ok(h, 1));
  return cx_rap_level_ms(h, out, n, "mg_rap_CF64");
}
int mg_rap_level_ms_CF32(mg_hierarchy* h, double* out, long long n) {
  MG_TRY(cx_level_ok(h, 1, CX_WANT32));
  return cx_rap_level_ms(h, out, n, "mg_rap_CF32");
}

// adjointHierarchy (MGsetup.jl:274-318 for complex VAL) on the resident hierarchy, in HBM: see include/mgvcycle.h
int mg_adjoint_hierarchy_CF64(mg_hierarchy* h) {
  MG_TRY(cx_handle_ok(h, CX_WANT64));   // (a null handle is answered without touching the device)
  UploadFence upload_fence;
  return cx_adjoint_hierarchy(h, CX_WANT64);
}
int mg_adjoint_hierarchy_CF32(mg_hierarchy* h) {
  MG_TRY(cx_handle_ok(h, CX_WANT32));
  UploadFence upload_fence;
  return cx_adjoint_hierarchy(h, CX_WANT32);
}

int mg_get_values_CF64(mg_hierarchy* h, long long level, long long which, double* out, long long nnz) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  if (!out) return fail(MG_ERR_INVALID, "null argument");
  MG_CF32_UNSUPPORTED(h);
  return cx_get_values<double>(h, level, which, out, nnz, CX_WANT64);
}
int mg_get_values_CF32(mg_hierarchy* h, long long level, long long which, float* out, long long nnz) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  if (!out) return fail(MG_ERR_INVALID, "null argument");
  return cx_get_values<float>(h, level, which, out, nnz, CX_WANT32);
}

int mg_get_relax_CF64(mg_hierarchy* h, long long level, double* out, long long n) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  if (!out) return fail(MG_ERR_INVALID, "null argument");
  MG_CF32_UNSUPPORTED(h);
  return cx_get_relax<double>(h, level, out, n, CX_WANT64);
}
int mg_get_relax_CF32(mg_hierarchy* h, long long level, float* out, long long n) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  if (!out) return fail(MG_ERR_INVALID, "null argument");
  return cx_get_relax<float>(h, level, out, n, CX_WANT32);
}

int mg_replace_values_CF64(mg_hierarchy* h, long long level, long long which, const double* nzval, long long nnz) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  if (!nzval) return fail(MG_ERR_INVALID, "null argument");
  MG_CF32_UNSUPPORTED(h);
  return cx_replace_values<double>(h, level, which, nzval, nnz, CX_WANT64);
}
// (a CF32 handle keeps widened copies of two operators: that of the coarsest one for the GMRES coarsest solve follows the new values
// here, that of As[1] for the Krylov drivers is dropped and widened again by the next driver call)
int mg_replace_values_CF32(mg_hierarchy* h, long long level, long long which, const float* nzval, long long nnz) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  if (!nzval) return fail(MG_ERR_INVALID, "null argument");
  MG_TRY(cx_replace_values<float>(h, level, which, nzval, nnz, CX_WANT32));
  CxState& S = *h->cx;
  if (which != MG_OP_A) return MG_OK;
  if (level == 1 && S.K_auto) {
    S.K.release();
    S.K_auto = false;
  }
  if (level == h->nlevels && S.coarse_gmres && S.cgA.set) {
    MG_TRY(cx_widen_values(h, S.lev[(size_t)level - 1].A, S.cgA));
    HIP_TRY(spin_sync(h->play->stream));
  }
  return MG_OK;
}

int mg_replace_krylov_values_CFP64(mg_hierarchy* h, const double* nzval, long long nnz) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  if (!nzval) return fail(MG_ERR_INVALID, "null argument");
  MG_TRY(cx_level_ok(h, 1, CX_ANY));
  CxState& S = *h->cx;
  if (!S.K.set || S.K_auto) return fail(MG_ERR_STATE, "no Krylov operator set (mg_set_krylov_operator_CFP64_INT64)");
  if (nnz != S.K.nnz) return fail(MG_ERR_INVALID, "nnz=%lld differs from the Krylov operator's pattern (%lld)", nnz, S.K.nnz);
  (void)hipSetDevice(h->device);
  return cx_write_values(h, S.K, nzval);
}

}  // extern "C"
