// mg_cabi.inc - part of libmgvcycle.so's single translation unit (included by mgvcycle.hip in this order; not compiled on its own).
// The C ABI of the single-GPU hierarchy (include/mgvcycle.h): create / set / finalize / cycle / solve / Krylov / measurement, stand-alone operators, the factor applier, hybrid Kaczmarz,
// and of its ghost-layer form (mg_ghost_*).

// ---- shared preambles and staging of the entry points (the value-type guards stay in the entry points: they name them) ----
namespace {
// Level `level` (1-based) of a handle: MG_ERR_INVALID for a null handle or a level outside 1..nlevels
int find_level(mg_hierarchy* h, long long level, Level** L) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  if (level < 1 || level > h->nlevels) return fail(MG_ERR_INVALID, "bad level %lld", level);
  *L = &h->lev[(size_t)level - 1];
  return MG_OK;
}

// Operator `which` (MG_OP_A / _P / _R) of level `level`: MG_ERR_INVALID for a null handle or an operator that was not set
int find_op(mg_hierarchy* h, long long level, long long which, Csr** M) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  *M = pick(h, level, which);
  if (!*M || !(*M)->set) return fail(MG_ERR_INVALID, "operator (level=%lld, which=%lld) not set", level, which);
  return MG_OK;
}

int need_finalized(mg_hierarchy* h) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  if (!h->finalized) return fail(MG_ERR_STATE, "hierarchy not finalized");
  return MG_OK;
}

// the caller's initial guess into the staging buffer: x == 0 (the usual call) is a device memset instead of n*nrhs*8
// bytes over PCIe (the scan of a zero vector runs at memory speed: host_all_zero)
int upload_x_or_zero(mg_hierarchy* h, const double* x, long long n, long long nrhs) {
  const long long len = n * nrhs;
  if (host_all_zero(x, len)) {
    HIP_TRY(hipMemsetAsync(h->stage_x.p, 0, sizeof(double) * (size_t)len, h->play->stream));
    return MG_OK;
  }
  return upload_block(h, x, h->stage_x.p, n, nrhs);
}

// How staged() puts the caller's x on the device: upload_x_or_zero (the drivers that read x), or as mg_cycle_FP64 decided -
// uploaded, or not at all when the cycle starts from x = 0
enum class StageX { or_zero, upload, skip };

// The host-pointer form of a device routine (b, x: column-major n x nrhs host blocks): b and x into the staging buffers,
// run(stage_b, stage_x), x back, the profile.  The caller has checked the arguments and set the device.
template <typename Run>
int staged(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs, StageX xs, Run run) {
  MG_TRY(upload_block(h, b, h->stage_b.p, n, nrhs));
  if (xs == StageX::or_zero) MG_TRY(upload_x_or_zero(h, x, n, nrhs));
  if (xs == StageX::upload) MG_TRY(upload_block(h, x, h->stage_x.p, n, nrhs));
  MG_TRY(run(h->stage_b.p, h->stage_x.p));
  MG_TRY(download_block(h, h->stage_x.p, x, n, nrhs));
  prof_collect(h);
  return MG_OK;
}

// A Krylov entry point: check_ready and the arguments, then run(b, x) - the device form on the caller's vectors (sharded handles
// too: the ghost-layer form runs the sharded drivers of mg_krylov.inc), the host form on the staging buffers
template <typename Run>
int krylov(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs, long long maxIter, bool device_form, Run run) {
  MG_TRY(check_ready(h, n, nrhs, /*sharded_ok=*/device_form));
  if (!b || !x || maxIter < 0) return fail(MG_ERR_INVALID, "null vector or maxIter < 0");
  (void)hipSetDevice(h->device);
  if (!device_form) return staged(h, b, x, n, nrhs, StageX::or_zero, run);
  MG_TRY(run(b, x));
  prof_collect(h);
  return MG_OK;
}

// One pass of the real drivers on the caller's vectors (mg_kry_*_dev_FP64): a finalized real FP64 handle whose drivers are not sharded
// (MG_ERR_STATE otherwise), n >= 1 of the caller's choosing.  A refusal launches nothing.
int kry_pass_ready(mg_hierarchy* h, long long n, const char* who) {
  if (!h) return fail(MG_ERR_INVALID, "%s: null hierarchy handle", who);
  if (h->cx) return fail(MG_ERR_STATE, "%s: FP64 entry point called on a complex handle", who);
  if (!h->finalized) return fail(MG_ERR_STATE, "%s: hierarchy not finalized", who);
  if (h->ghost) return fail(MG_ERR_STATE, "%s: this handle is one rank's part of a sharded hierarchy, its drivers' sums span all ranks", who);
  if (n < 1) return fail(MG_ERR_INVALID, "%s: n=%lld", who, n);
  (void)hipSetDevice(h->device);
  return MG_OK;
}

// device_id a visible device, made current (the create entry points)
int use_device(long long device_id) {
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (ndev <= 0) return fail(MG_ERR_HIP, "no HIP device visible: the multigrid cycle has no CPU fallback");
  if (device_id < 0 || device_id >= ndev) return fail(MG_ERR_INVALID, "device_id=%lld but %d devices visible", device_id, ndev);
  HIP_TRY(hipSetDevice((int)device_id));
  return MG_OK;
}
// The explicit inverse of the resident coarsest operator, built in HBM (mg_dense_inv.hpp) (mg_build_coarse_dense_inverse_FP64, mg_rap_FP64).
// coarse_inverse_check: what is refused before the first write; coarse_inverse_finish (behind the caller's synchronisation): the
// flag read, the spare buffer exchanged with Ainv when it is clean.
int coarse_inverse_check(mg_hierarchy* h) {
  if (h->ghost) return fail(MG_ERR_UNSUPPORTED, "the device inverse is not served for a sharded hierarchy");
  const Csr& A = h->lev[(size_t)h->nlevels - 1].A;
  if (!A.set) return fail(MG_ERR_STATE, "the coarsest operator was not uploaded");
  if (A.wide) return fail(MG_ERR_UNSUPPORTED, "the coarsest operator holds 64-bit row pointers: the device inverse serves int32 operators");
  if (A.n_rows != A.n_cols) return fail(MG_ERR_INVALID, "the coarsest operator is %lld x %lld", A.n_rows, A.n_cols);
  if (A.n_rows > dense_inv_max(h->opt))
    return fail(MG_ERR_UNSUPPORTED, "the coarsest operator has %lld rows: the device inverse serves up to %lld (option coarse_device_inverse_max)",
                A.n_rows, dense_inv_max(h->opt));
  return MG_OK;
}
int coarse_inverse_finish(mg_hierarchy* h, DenseInv<double>& K, DevBuf<double>& spare, const char* who) {
  int col = 0;
  const int rc = K.singular_column(&col);
  if (rc != MG_OK || col != 0) {
    spare.release();
    return rc != MG_OK ? rc
                       : fail(MG_ERR_INVALID, "%s: the coarsest operator is singular to working precision (zero or non-finite pivot in column %d): the previous inverse stays",
                              who, col);
  }
  std::swap(h->Ainv, spare);
  spare.release();
  return MG_OK;
}

}  // namespace

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

const char* mg_last_error(void) { return g_err.c_str(); }
const char* mg_version(void) { return "mgvcycle 0.1 (gfx950, fp64, csr-stream)"; }

int mg_create(long long nlevels, long long nrhs, long long device_id, mg_hierarchy** out) {
  if (!out) return fail(MG_ERR_INVALID, "out is null");
  *out = nullptr;
  if (nlevels < 1 || nlevels > 64) return fail(MG_ERR_INVALID, "nlevels=%lld out of range [1,64]", nlevels);
  if (nrhs < 1) return fail(MG_ERR_INVALID, "nrhs=%lld must be >= 1", nrhs);
  MG_TRY(use_device(device_id));
  mg_hierarchy* h = new mg_hierarchy();
  h->opt = Options::from_env();   // the only place the environment is read for this handle
  h->device = (int)device_id;
  h->nlevels = nlevels;
  h->nrhs = nrhs;
  h->lev.resize((size_t)nlevels);
  h->slots.resize((size_t)nlevels * MG_K_COUNT);
  hipError_t e = hipStreamCreateWithFlags(&h->lane0.stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete h;
    return fail(MG_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
  }
  if (h->lane0.partial.alloc((size_t)h->nred_blocks) != MG_OK || h->lane0.partial2.alloc(256) != MG_OK || h->lane0.scalar.alloc(1) != MG_OK ||
      hipHostMalloc(reinterpret_cast<void**>(&h->h_scalar), 4 * sizeof(double)) != hipSuccess) {
    mg_destroy(h);
    return fail(MG_ERR_HIP, "allocation of reduction scratch failed");
  }
  *out = h;
  return MG_OK;
}

// replaceMatrixInHierarchy on the device (MGsetup.jl:226-270): new fine values (same sparsity), then per level
// relaxPrecs[l] = getRelaxPrec(As[l]) and As[l+1] = Ps[l]*As[l]*Rs[l] on the fixed patterns.  With the option
// coarse_device_inverse and a dense inverse installed, the new coarsest operator's inverse is built in HBM behind the
// last Galerkin product, inside the same synchronisation (mg_dense_inv.hpp; a singular operator is an error return
// and the previous inverse stays).  Otherwise the coarsest factorisation stays with the host: fetch the coarsest
// values with mg_get_values_FP64, factor, hand the inverse back with mg_set_coarse_dense_inverse_FP64 and call mg_finalize.
int mg_rap_FP64(mg_hierarchy* h, const double* fine_nzval, long long nnz, long long relaxKind,
                const double* omega, long long* levels_done) {
  MG_CF64_UNSUPPORTED(h);
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  graphs_clear(h);
  if (!h->finalized) return fail(MG_ERR_STATE, "hierarchy not finalized");
  if (h->ghost) return fail(MG_ERR_UNSUPPORTED, "the numeric Galerkin product of a sharded hierarchy needs the ghost rows of the new operator: every rank rebuilds and re-uploads its part");
  if (!fine_nzval || !omega) return fail(MG_ERR_INVALID, "null argument");
  if (relaxKind != 0 && relaxKind != 1) return fail(MG_ERR_INVALID, "relaxKind must be 0 (Jac) or 1 (SPAI)");
  Level& L0 = h->lev[0];
  if (nnz != L0.A.nnz) return fail(MG_ERR_INVALID, "nnz=%lld differs from the stored fine pattern (%lld)", nnz, L0.A.nnz);
  (void)hipSetDevice(h->device);
  const int nl = (int)h->nlevels;
  for (int l = 0; l < nl; ++l)
    if (h->lev[(size_t)l].A.wide || h->lev[(size_t)l].P.wide || h->lev[(size_t)l].R.wide)
      return fail(MG_ERR_UNSUPPORTED, "level %d holds an operator with 64-bit row pointers (>= 2^31 non-zeros): the numeric Galerkin product on the device serves int32 operators", l + 1);
  for (int l = 1; l < nl; ++l)
    if (!h->lev[(size_t)l].A.rows_sorted)
      return fail(MG_ERR_UNSUPPORTED, "As[%d] holds a row whose stored columns do not ascend: the numeric Galerkin product on the device finds its target columns by binary search (sort the rows, or take the host path)", l + 1);
  const bool dev_inverse = h->opt.coarse_device_inverse && h->coarse_set && !h->coarse_lu && !h->coarse_gmres && !h->coarse_dd && h->Ainv.p;
  if (dev_inverse) MG_TRY(coarse_inverse_check(h));
  HIP_TRY(spin_sync(h->play->stream));
  HIP_TRY(hipMemcpyAsync(L0.A.val.p, fine_nzval, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, h->play->stream));
  for (int l = 0; l + 1 < nl; ++l) {
    Level& L = h->lev[(size_t)l];
    Level& C = h->lev[(size_t)l + 1];
    const int nb = (int)((L.n + mgk::BLK - 1) / mgk::BLK);
    if (relaxKind == 0) {
      hipLaunchKernelGGL(mgk::relax_jacobi, dim3(nb), dim3(mgk::BLK), 0, h->play->stream, L.A.dev(), omega[l], L.d.p);
    } else {
      MG_TRY(build_transposed_pattern(L.A));   // (first SPAI re-setup of this level only)
      hipLaunchKernelGGL(mgk::colsumsq_kernel, dim3(nb), dim3(mgk::BLK), 0, h->play->stream, L.A.val.p, L.A.t_ptr.p, L.A.t_perm.p,
                         (int)L.A.n_cols, h->play->lev[(size_t)l].r.p);   // the level's r as scratch for the column sums
      hipLaunchKernelGGL(mgk::relax_spai, dim3(nb), dim3(mgk::BLK), 0, h->play->stream, L.A.dev(), omega[l], h->play->lev[(size_t)l].r.p, L.d.p);
    }
    hipLaunchKernelGGL(mgk::rap_numeric, dim3((unsigned)C.n), dim3(64), 0, h->play->stream, L.R.dev(), L.A.dev(), L.P.dev(),
                       C.A.rowptr.p, C.A.colidx.p, C.A.val.p, (int)std::max<long long>(1, std::min<long long>(h->opt.rap_chunk, mgk::RAP_CAP)));
    HIP_TRY(hipGetLastError());
  }
  DenseInv<double> inv;      // option coarse_device_inverse: the new coarsest operator's inverse, into a spare buffer (exchanged below)
  DevBuf<double> inv_spare;
  int inv_rc = MG_OK;
  if (dev_inverse) {
    const Csr& Ac = h->lev[(size_t)nl - 1].A;
    inv_rc = coarse_inverse_enqueue<double, double>(inv, inv_spare, Ac.n_rows, Ac.rowptr.p, Ac.colidx.p, Ac.val.p, h->play->stream);
  }
  const hipError_t synced = spin_sync(h->play->stream);
  if (synced != hipSuccess || inv_rc != MG_OK) {
    inv_spare.release();
    if (inv_rc != MG_OK) return inv_rc;
    HIP_TRY(synced);
  }
  if (dev_inverse) inv_rc = coarse_inverse_finish(h, inv, inv_spare, "mg_rap_FP64");
  // row-class dictionaries follow the new values (coarse values come back from HBM; rap_numeric adds every entry in a
  // fixed order, so rows that were bit-identical before a constant-coefficient update still are afterwards)
  MG_TRY(refresh_rowclasses(&L0.A, fine_nzval));
  for (int l = 1; l < nl; ++l) {
    Csr& Ac = h->lev[(size_t)l].A;
    if (!Ac.has_rc) continue;
    std::vector<double> hv((size_t)Ac.nnz);
    HIP_TRY(hipMemcpy(hv.data(), Ac.val.p, hv.size() * sizeof(double), hipMemcpyDeviceToHost));
    MG_TRY(refresh_rowclasses(&Ac, hv.data()));
  }
  for (int l = 0; l + 1 < nl; ++l) MG_TRY(derive_class_d(h->lev[(size_t)l]));   // relaxPrecs were recomputed above
  for (int l = 0; l < nl; ++l) {   // tile / march tables follow the new classes
    MG_TRY(build_staged(h->lev[(size_t)l].A, h->lev[(size_t)l].grid));
    MG_TRY(build_small27(h->lev[(size_t)l].A, h->lev[(size_t)l].grid, h->lev[(size_t)l].d.p, h->lev[(size_t)l].relax_set && l + 1 < nl));
    MG_TRY(build_band27(h->lev[(size_t)l].A, h->lev[(size_t)l].grid));   // (the planar values follow the new ones: one fill kernel)
  }
  if (levels_done) *levels_done = nl - 1;
  return inv_rc;   // (a singular coarsest operator: the operators hold the new values, the coarsest solve the previous inverse)
}

int mg_get_values_FP64(mg_hierarchy* h, long long level, long long which, double* out, long long nnz) {
  MG_REAL_ONLY(h);
  Csr* M;
  MG_TRY(find_op(h, level, which, &M));
  if (!out || nnz != M->nnz) return fail(MG_ERR_INVALID, "nnz=%lld differs from the stored pattern (%lld)", nnz, M->nnz);
  (void)hipSetDevice(h->device);
  HIP_TRY(spin_sync(h->play->stream));
  HIP_TRY(hipMemcpy(out, M->val.p, (size_t)nnz * sizeof(double), hipMemcpyDeviceToHost));
  return MG_OK;
}

int mg_get_relax_FP64(mg_hierarchy* h, long long level, double* out, long long n) {
  MG_REAL_ONLY(h);
  Level* L;
  MG_TRY(find_level(h, level, &L));
  if (!out || !L->relax_set || n != (long long)L->d.n) return fail(MG_ERR_INVALID, "relaxPrecs[%lld] not set or wrong length", level);
  (void)hipSetDevice(h->device);
  HIP_TRY(spin_sync(h->play->stream));
  HIP_TRY(hipMemcpy(out, L->d.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  return MG_OK;
}

int mg_destroy(mg_hierarchy* h) {
  if (!h) return MG_OK;
  graphs_clear(h);
  (void)hipSetDevice(h->device);
  if (h->play->stream) (void)spin_sync(h->play->stream);
  dd_detach(h);   // (a borrowed Schwarz handle stays its owner's)
  if (h->ghost) { gh_release(h->ghost); h->ghost = nullptr; }
  if (h->cx) { cx_destroy(h->cx); h->cx = nullptr; }
  prof_collect(h);
  for (auto e : h->ev_pool) (void)hipEventDestroy(e);
  for (auto& L : h->lev) {
    if (L.vanka) { L.vanka->release(); delete L.vanka; L.vanka = nullptr; }
    L.A.release();
    L.P.release();
    L.R.release();
    L.d.release();
    L.x2.release();
    L.x3.release();
  }
  h->m3sink.release();
  h->Ainv.release();
  for (DevBuf<int>* d : {&h->luLptr, &h->luLcol, &h->luUptr, &h->luUcol, &h->luP, &h->luQ, &h->luLorder, &h->luLlvl,
                         &h->luUorder, &h->luUlvl})
    d->release();
  h->luLval.release();
  h->luUval.release();
  h->luWork.release();
  h->luInvL.release(); h->luInvU.release(); h->luTail.release(); h->luLslot.release(); h->luUslot.release();
  h->kwc.release();
  h->coarse_d.release();
  h->stage_b.release();
  h->stage_x.release();
  h->stage_t.release();
  h->kr.release();
  h->kz.release();
  h->kp.release();
  h->kAp.release();
  h->kw.release();
  if (h->h_scalar) (void)hipHostFree(h->h_scalar);
  if (h->h_cols) (void)hipHostFree(h->h_cols);
  for (auto& cb : h->colbuf) cb.release();
  for (hipEvent_t e : h->lane_ready) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t& e : h->pipe_ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
  if (h->h_blk) (void)hipHostFree(h->h_blk);
  if (h->h_kscal) (void)hipHostFree(h->h_kscal);
  if (h->h_blk_c) (void)hipHostFree(h->h_blk_c);
  h->blk_partial.release();
  h->blk_c.release();
  h->lane0.release();
  for (Play* p : h->lanes) {
    p->release();
    delete p;
  }
  delete h;
  return MG_OK;
}

int mg_set_operator_FP64_INT64(mg_hierarchy* h, long long level, long long which, long long n_rows,
                               long long n_cols, const long long* colptr, const long long* rowval,
                               const double* nzval) {
  UploadFence upload_fence;
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  if (h->cx) return cx_set_transfer(h, level, which, n_rows, n_cols, colptr, rowval, nzval);   // P, R of a CF64 handle (real)
  graphs_clear(h);
  Csr* M = pick(h, level, which);
  if (!M) return fail(MG_ERR_INVALID, "bad (level=%lld, which=%lld)", level, which);
  if ((which == MG_OP_P || which == MG_OP_R) && level == h->nlevels)
    return fail(MG_ERR_INVALID, "the coarsest level %lld has no transfer operators", level);
  (void)hipSetDevice(h->device);
  MG_TRY(upload_csr(M, h->opt, n_rows, n_cols, colptr, rowval, nzval));
  h->finalized = false;
  return MG_OK;
}

int mg_set_relax_FP64(mg_hierarchy* h, long long level, const double* d, long long n,
                      long long relaxPre, long long relaxPost) {
  MG_REAL_ONLY(h);
  UploadFence upload_fence;
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  graphs_clear(h);
  Level* L;
  MG_TRY(find_level(h, level, &L));
  if (!d || n < 1) return fail(MG_ERR_INVALID, "empty relaxPrec");
  if (relaxPre < 0 || relaxPost < 0) return fail(MG_ERR_INVALID, "negative sweep count");
  (void)hipSetDevice(h->device);
  MG_TRY(L->d.alloc((size_t)n));
  HIP_TRY(hipMemcpy(L->d.p, d, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  L->relax_set = true;
  L->A.rc_has_d = false;   // re-derived by mg_finalize
  L->A.sm_ok = false;      // (its records carry the relaxPrec: rebuilt by mg_finalize)
  L->npre = relaxPre;
  L->npost = relaxPost;
  h->finalized = false;
  return MG_OK;
}

// Override one format-selection switch of this handle (the names of DESIGN.md's table without the MG_ prefix, lower
// case: "no_rowclass", "no_tile", "tile_min_wg", ...).  Takes effect for operators uploaded afterwards and for the next
// mg_finalize; call it right after mg_create.
int mg_set_option(mg_hierarchy* h, const char* key, double value) {
  if (!h || !key) return fail(MG_ERR_INVALID, "null argument");
  graphs_clear(h);
  if (!h->opt.set(key, value)) return fail(MG_ERR_INVALID, "unknown option '%s'", key);
  for (auto& L : h->lev) {
    L.A.opt = h->opt;
    L.P.opt = h->opt;
    L.R.opt = h->opt;
  }
  h->finalized = false;
  return MG_OK;
}

int mg_graph_launches(mg_hierarchy* h, long long* launches, long long* graphs) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  if (launches) *launches = h->graph_launches;
  if (graphs) *graphs = (long long)h->graphs.size();
  return MG_OK;
}

int mg_set_grid_hint(mg_hierarchy* h, long long level, long long n1, long long n2, long long n3) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  graphs_clear(h);
  Level* L;
  MG_TRY(find_level(h, level, &L));
  if (n1 < 1 || n2 < 1 || n3 < 1) return fail(MG_ERR_INVALID, "grid dimensions must be >= 1");
  L->grid[0] = n1;
  L->grid[1] = n2;
  L->grid[2] = n3;
  h->finalized = false;
  return MG_OK;
}

int mg_set_relax_type(mg_hierarchy* h, long long relaxType) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  graphs_clear(h);
  if (relaxType != 0 && relaxType != 1 && relaxType != 2) return fail(MG_ERR_INVALID, "relaxType must be 0 (Jac/SPAI), 1 (Jac-GMRES) or 2 (Vanka)");
  if (h->cx && relaxType == 1) return fail(MG_ERR_UNSUPPORTED, "relaxation type 1 (Jac-GMRES) is not served for CF64 handles");
  if (h->cx && relaxType == 2) return fail(MG_ERR_UNSUPPORTED, "relaxation type 2 (Vanka) is not served for CF64 handles");
  h->relax_type = (int)relaxType;
  h->finalized = false;
  return MG_OK;
}

// The Vanka blocks of one level (relaxation type 2), built from the operator the level already holds
int mg_set_vanka_FP64(mg_hierarchy* h, long long level, long long dim, const long long* n, long long includePressure,
                      long long VankaType, const float* D_blocks) {
  MG_CF64_UNSUPPORTED(h);
  UploadFence upload_fence;
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  graphs_clear(h);
  Level* L;
  MG_TRY(find_level(h, level, &L));
  if (!L->A.set) return fail(MG_ERR_STATE, "As[%lld] was not set: upload the operator before its Vanka blocks", level);
  if (L->A.wide) return fail(MG_ERR_UNSUPPORTED, "operators with 64-bit row pointers are not served by the Vanka smoother");
  if (L->A.n_rows != L->A.n_cols) return fail(MG_ERR_INVALID, "As[%lld] is not square", level);
  MG_TRY(vanka_type_served(VankaType));
  mgk::VankaGeo G;
  MG_TRY(vanka_geometry(dim, n, includePressure, L->A.n_rows, &G));
  (void)hipSetDevice(h->device);
  if (h->play->stream) HIP_TRY(spin_sync(h->play->stream));
  if (L->vanka) { L->vanka->release(); delete L->vanka; L->vanka = nullptr; }
  VankaCore* V = new VankaCore();
  const int rc = vanka_core_init(V, false, G, D_blocks);
  if (rc != MG_OK) {
    V->release();
    delete V;
    return rc;
  }
  L->vanka = V;
  L->vanka_type = (int)VankaType;
  h->finalized = false;
  return MG_OK;
}

int mg_set_cycle_type(mg_hierarchy* h, long long cycleType) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  if (cycleType != 'V' && cycleType != 'W' && cycleType != 'F' && cycleType != 'K')
    return fail(MG_ERR_INVALID, "cycleType must be 'V', 'W', 'F' or 'K'");
  if (h->cx && cycleType == 'K') return fail(MG_ERR_UNSUPPORTED, "cycle 'K' is not served for CF64 handles");
  if (h->cycle == (char)cycleType) return MG_OK;   // (the cycle type is part of the graph key: nothing to drop)
  graphs_clear(h);
  if ((cycleType == 'K') != (h->cycle == 'K')) h->finalized = false;  // memKcycle must be (de)allocated
  h->cycle = (char)cycleType;
  return MG_OK;
}

int mg_set_coarse_dense_inverse_FP64(mg_hierarchy* h, long long n, const double* Ainv) {
  MG_REAL_ONLY(h);
  UploadFence upload_fence;
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  graphs_clear(h);
  if (n < 1 || !Ainv) return fail(MG_ERR_INVALID, "empty coarse inverse");
  if (n > 46000) return fail(MG_ERR_UNSUPPORTED, "dense coarse inverse of order %lld is too large", n);
  (void)hipSetDevice(h->device);
  // column-major -> row-major on the host (one-off, setup time)
  std::vector<double> rm((size_t)n * (size_t)n);
  for (long long j = 0; j < n; ++j)
    for (long long i = 0; i < n; ++i) rm[(size_t)i * n + j] = Ainv[(size_t)j * n + i];
  MG_TRY(h->Ainv.alloc(rm.size()));
  HIP_TRY(hipMemcpy(h->Ainv.p, rm.data(), rm.size() * sizeof(double), hipMemcpyHostToDevice));
  dd_detach(h);
  h->n_coarse = n;
  h->coarse_set = true;
  h->coarse_lu = false;
  h->coarse_gmres = false;
  h->finalized = false;
  return MG_OK;
}

int mg_build_coarse_dense_inverse_FP64(mg_hierarchy* h) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  MG_REAL_ONLY(h);
  MG_TRY(coarse_inverse_check(h));
  graphs_clear(h);
  (void)hipSetDevice(h->device);
  const Csr& A = h->lev[(size_t)h->nlevels - 1].A;
  DenseInv<double> K;
  DevBuf<double> spare;
  int rc = coarse_inverse_enqueue<double, double>(K, spare, A.n_rows, A.rowptr.p, A.colidx.p, A.val.p, h->play->stream);
  if (spin_sync(h->play->stream) != hipSuccess && rc == MG_OK) rc = fail(MG_ERR_HIP, "mg_build_coarse_dense_inverse_FP64: stream failed");
  if (rc != MG_OK) {
    spare.release();
    return rc;
  }
  MG_TRY(coarse_inverse_finish(h, K, spare, "mg_build_coarse_dense_inverse_FP64"));
  dd_detach(h);
  h->n_coarse = A.n_rows;
  h->coarse_set = true;
  h->coarse_lu = false;
  h->coarse_gmres = false;
  h->finalized = false;
  return MG_OK;
}

int mg_get_coarse_dense_inverse_FP64(mg_hierarchy* h, long long n, double* out) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  MG_REAL_ONLY(h);
  if (!out) return fail(MG_ERR_INVALID, "null argument");
  if (!h->coarse_set || h->coarse_lu || h->coarse_gmres || h->coarse_dd || !h->Ainv.p)
    return fail(MG_ERR_STATE, "the coarsest solve of this handle is not a dense inverse");
  if (n != h->n_coarse) return fail(MG_ERR_INVALID, "n=%lld differs from the coarsest order %lld", n, h->n_coarse);
  (void)hipSetDevice(h->device);
  HIP_TRY(spin_sync(h->play->stream));
  return dense_inverse_readback<1>(h->Ainv, n, out);
}

int mg_dense_inverse_FP64(long long device, long long n, const double* A, double* out) {
  MG_TRY(dense_inverse_args(n, A, out, "mg_dense_inverse_FP64"));
  MG_TRY(use_device(device));
  return dense_inverse_host<double>(n, A, out, "mg_dense_inverse_FP64");
}

// Coarsest solve from sparse LU factors in the layout of the reference's native applier (deps/src/parLU.cpp:120-190;
// produced by setupLUFactor, parallelJuliaSolver.jl:113-148): CSR L (diagonal last in each row) and U (diagonal first),
// 1-based Int64 row pointers / column indices, permutations p, q with A[p,q] = L*U, i.e. x[q] = U \ (L \ b[p]).
int mg_set_coarse_lu_FP64_INT64(mg_hierarchy* h, long long n, const long long* Lptr, const long long* Lcol,
                                const double* Lval, const long long* Uptr, const long long* Ucol,
                                const double* Uval, const long long* p, const long long* q) {
  MG_REAL_ONLY(h);
  UploadFence upload_fence;
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  graphs_clear(h);
  if (n < 1 || !Lptr || !Lcol || !Lval || !Uptr || !Ucol || !Uval || !p || !q) return fail(MG_ERR_INVALID, "null or empty factor");
  if (n >= (1LL << 31) - 1 || Lptr[n] - 1 >= (1LL << 31) || Uptr[n] - 1 >= (1LL << 31))
    return fail(MG_ERR_UNSUPPORTED, "factors exceed int32 device indices");
  (void)hipSetDevice(h->device);
  const size_t N = (size_t)n;
  auto levels = [&](const std::vector<int>& P, const std::vector<int>& Cc, bool lower, int M, std::vector<int>& order,
                    std::vector<int>& lvlptr) { lu_levels(n, P, Cc, lower, M, order, lvlptr); };
  auto conv = [&](const long long* ptr, const long long* col, bool lower, std::vector<int>& P, std::vector<int>& Cc,
                  std::vector<int>& order, std::vector<int>& lvlptr) -> int { return lu_convert(n, ptr, col, lower, P, Cc, order, lvlptr); };
  std::vector<int> LP, LC, LO, LL, UP, UC, UO, UL, pp(N), qq(N);
  MG_TRY(conv(Lptr, Lcol, true, LP, LC, LO, LL));
  MG_TRY(conv(Uptr, Ucol, false, UP, UC, UO, UL));
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
  MG_TRY(up_i(h->luLptr, LP)); MG_TRY(up_i(h->luLcol, LC)); MG_TRY(up_i(h->luLorder, LO)); MG_TRY(up_i(h->luLlvl, LL));
  MG_TRY(up_i(h->luUptr, UP)); MG_TRY(up_i(h->luUcol, UC)); MG_TRY(up_i(h->luUorder, UO)); MG_TRY(up_i(h->luUlvl, UL));
  MG_TRY(up_i(h->luP, pp)); MG_TRY(up_i(h->luQ, qq));
  MG_TRY(h->luLval.alloc(LC.size()));
  MG_TRY(h->luUval.alloc(UC.size()));
  HIP_TRY(hipMemcpy(h->luLval.p, Lval, LC.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->luUval.p, Uval, UC.size() * sizeof(double), hipMemcpyHostToDevice));
  h->nLlvl = (int)LL.size() - 1;
  h->nUlvl = (int)UL.size() - 1;
  // chip-wide form: the trailing chains of single-row levels (rows n-1, n-2, ... one per level: the dense last
  // supernode) are solved through the explicit inverse of their dense block
  h->lu_multi = n >= h->opt.lu_multi_min_rows;
  h->luML = h->luMU = 0;
  h->luInvL.release(); h->luInvU.release(); h->luTail.release();
  if (h->lu_multi) {
    // (the templated applier's cxlu_upload, mg_complex.inc, carries the same estimate with sizeof(value) bytes: keep the two in step)
    // Size M of the trailing block: a level costs ~8 us of dependent latency whatever its width, the dense product
    // 8*M^2/2 bytes of traffic per factor - take the candidate with the smallest estimate.  (33^3 Poisson level under
    // a minimum-degree ordering: 3284 levels per factor at M = 0, 639 at M = 4096, 132 at M = 8192.)
    const int cap = (int)std::min<long long>(h->opt.lu_dense_tail_max, n);
    int M = 0;
    double best = 0.0;
    std::vector<int> o, lp;
    for (int cand = 0; cand <= cap; cand = cand == 0 ? (int)std::max<long long>(h->opt.lu_dense_tail_min, 1) : cand * 2) {
      levels(LP, LC, true, cand, o, lp);
      double est = 8e-6 * (double)(lp.size() - 1);
      levels(UP, UC, false, cand, o, lp);
      est += 8e-6 * (double)(lp.size() - 1) + 2.0 * 4.0 * (double)cand * (double)cand / 4e12;
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
    levels(LP, LC, true, M, o, h->luLlvl_h);
    MG_TRY(slots(LP, true, o, h->luLslot));
    levels(UP, UC, false, M, o, h->luUlvl_h);
    MG_TRY(slots(UP, false, o, h->luUslot));
    const int ML = M, MU = M;
    auto invert = [&](bool lower, int M, const DevBuf<int>& ptr, const DevBuf<int>& col, const DevBuf<double>& val,
                      DevBuf<double>& inv) -> int {
      const int ld = (M + 63) / 64 * 64;
      DevBuf<double> D;
      MG_TRY(D.alloc((size_t)ld * (size_t)ld));
      MG_TRY(inv.alloc((size_t)ld * (size_t)ld));
      HIP_TRY(hipMemsetAsync(D.p, 0, (size_t)ld * (size_t)ld * sizeof(double), h->play->stream));
      hipLaunchKernelGGL(mgk::tri_gather_block, dim3((unsigned)(((long long)ld * 64 + mgk::BLK - 1) / mgk::BLK)), dim3(mgk::BLK),
                         0, h->play->stream, ptr.p, col.p, val.p, (int)n - M, M, ld, D.p);
      if (lower) hipLaunchKernelGGL(mgk::tri_inverse<true>, dim3((unsigned)(ld / 64)), dim3(256), 0, h->play->stream, D.p, inv.p, ld);
      else hipLaunchKernelGGL(mgk::tri_inverse<false>, dim3((unsigned)(ld / 64)), dim3(256), 0, h->play->stream, D.p, inv.p, ld);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipStreamSynchronize(h->play->stream));
      return MG_OK;
    };
    if (ML > 0) MG_TRY(invert(true, ML, h->luLptr, h->luLcol, h->luLval, h->luInvL));
    if (MU > 0) MG_TRY(invert(false, MU, h->luUptr, h->luUcol, h->luUval, h->luInvU));
    h->luML = ML;
    h->luMU = MU;
    if (h->opt.debug_format)
      std::fprintf(stderr, "[mgvcycle] coarse LU n=%lld: dense trailing block %d, L %zu levels ahead of it (%d in all), U %zu behind it (%d)\n",
                   n, M, h->luLlvl_h.size() - 1, h->nLlvl, h->luUlvl_h.size() - 1, h->nUlvl);
  }
  dd_detach(h);
  h->n_coarse = n;
  h->coarse_set = true;
  h->coarse_lu = true;
  h->coarse_gmres = false;
  h->Ainv.release();
  h->finalized = false;
  return MG_OK;
}

// Coarsest solve by Jacobi-preconditioned FGMRES (coarseSolveType "GMRES", MGcycle.jl:152-168): d = relaxParam ./ diag(A_c)
// as defineCoarsestAinv stores it in param.LU (MGsetup.jl:334).
int mg_set_coarse_gmres_FP64(mg_hierarchy* h, long long n, const double* d) {
  MG_CF64_UNSUPPORTED(h);
  UploadFence upload_fence;
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  graphs_clear(h);
  if (n < 1 || !d) return fail(MG_ERR_INVALID, "empty preconditioner");
  (void)hipSetDevice(h->device);
  MG_TRY(h->coarse_d.alloc((size_t)n));
  HIP_TRY(hipMemcpy(h->coarse_d.p, d, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  dd_detach(h);
  h->n_coarse = n;
  h->coarse_set = true;
  h->coarse_gmres = true;
  h->coarse_lu = false;
  h->Ainv.release();
  h->finalized = false;
  return MG_OK;
}

int mg_finalize(mg_hierarchy* h) {
  UploadFence upload_fence;
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  if (h->cx) return cx_finalize(h);
  graphs_clear(h);
  (void)hipSetDevice(h->device);
  const int nl = (int)h->nlevels;
  for (int l = 0; l < nl; ++l) {
    Level& L = h->lev[l];
    if (h->lu_only && nl == 1 && !L.A.set) {   // mg_lu_*: no operator, only the factors
      L.n = h->n_coarse;
      continue;
    }
    if (!L.A.set) return fail(MG_ERR_STATE, "As[%d] was not set", l + 1);
    if (L.A.n_rows != L.A.n_cols) return fail(MG_ERR_INVALID, "As[%d] is not square", l + 1);
    L.n = L.A.n_rows;
    if (l < nl - 1) {
      if (!L.P.set || !L.R.set) return fail(MG_ERR_STATE, "Ps[%d]/Rs[%d] were not set", l + 1, l + 1);
      if (!L.relax_set) return fail(MG_ERR_STATE, "relaxPrecs[%d] was not set", l + 1);
      if ((long long)L.d.n != L.n) return fail(MG_ERR_INVALID, "relaxPrecs[%d] has length %zu, expected %lld", l + 1, L.d.n, L.n);
    }
  }
  for (int l = 0; l < nl - 1; ++l) {
    Level& L = h->lev[l];
    const long long nc = h->lev[l + 1].A.n_rows;
    if (L.P.n_rows != L.n || L.P.n_cols != nc)
      return fail(MG_ERR_INVALID, "Ps[%d] is %lldx%lld, expected %lldx%lld", l + 1, L.P.n_rows, L.P.n_cols, L.n, nc);
    if (L.R.n_rows != nc || L.R.n_cols != L.n)
      return fail(MG_ERR_INVALID, "Rs[%d] is %lldx%lld, expected %lldx%lld", l + 1, L.R.n_rows, L.R.n_cols, nc, L.n);
  }
  if (h->relax_type == 2)
    for (int l = 0; l < nl - 1; ++l) {
      const Level& L = h->lev[(size_t)l];
      if (!L.vanka) return fail(MG_ERR_STATE, "relaxation type 2 (Vanka) is set, but level %d has no blocks (mg_set_vanka_FP64)", l + 1);
      if (L.vanka->G.N != L.n) return fail(MG_ERR_INVALID, "the Vanka blocks of level %d serve %d unknowns, As[%d] has %lld rows", l + 1, L.vanka->G.N, l + 1, L.n);
    }
  if (!h->coarse_set) return fail(MG_ERR_STATE, "the coarsest solve was not set");
  if (h->n_coarse != h->lev[nl - 1].n)
    return fail(MG_ERR_INVALID, "coarse inverse order %lld != coarsest level size %lld", h->n_coarse, h->lev[nl - 1].n);
  if (h->coarse_dd && h->nrhs != 1)
    return fail(MG_ERR_UNSUPPORTED, "a Schwarz sweep as coarsest solve serves one right-hand side (nrhs=%lld): the reference's sweep indexes b[Idxs]", h->nrhs);
  for (int l = 0; l < nl - 1; ++l) MG_TRY(derive_class_d(h->lev[(size_t)l]));
  MG_TRY(alloc_scratch(h));

  h->finalized = true;
  return MG_OK;
}

int mg_set_nrhs(mg_hierarchy* h, long long nrhs) {
  UploadFence upload_fence;
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  graphs_clear(h);
  if (nrhs < 1) return fail(MG_ERR_INVALID, "nrhs must be >= 1");
  if (h->cx && nrhs != 1) return fail(MG_ERR_UNSUPPORTED, "CF64 handles serve one right-hand side (nrhs=%lld)", nrhs);
  if (nrhs == h->nrhs) return MG_OK;
  if (h->coarse_dd && nrhs != 1)
    return fail(MG_ERR_UNSUPPORTED, "a Schwarz sweep as coarsest solve serves one right-hand side (nrhs=%lld): the reference's sweep indexes b[Idxs]", nrhs);
  if (h->ghost && nrhs > 24) return fail(MG_ERR_UNSUPPORTED, "ghost-layer form: blocks of up to 24 columns (column-wise solve)");
  (void)hipSetDevice(h->device);
  h->nrhs = nrhs;
  if (h->finalized) {
    HIP_TRY(spin_sync(h->play->stream));
    MG_TRY(alloc_scratch(h));
  }
  return MG_OK;
}

int mg_replace_values_FP64(mg_hierarchy* h, long long level, long long which, const double* nzval,
                           long long nnz) {
  MG_REAL_ONLY(h);
  UploadFence upload_fence;
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  graphs_clear(h);
  Csr* M;
  MG_TRY(find_op(h, level, which, &M));
  if (nnz != M->nnz) return fail(MG_ERR_INVALID, "nnz=%lld differs from the stored pattern (%lld)", nnz, M->nnz);
  (void)hipSetDevice(h->device);
  HIP_TRY(spin_sync(h->play->stream));
  HIP_TRY(hipMemcpy(M->val.p, nzval, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice));
  MG_TRY(refresh_rowclasses(M, nzval));
  if (which == MG_OP_A) {
    Level& L = h->lev[(size_t)level - 1];
    if (L.relax_set) MG_TRY(derive_class_d(L));
    MG_TRY(build_staged(L.A, L.grid));
    MG_TRY(build_small27(L.A, L.grid, L.d.p, L.relax_set && level < h->nlevels));
    MG_TRY(build_band27(L.A, L.grid));
  }
  if (which == MG_OP_R && level < h->nlevels) MG_TRY(build_small_restrict(*M, h->lev[(size_t)level - 1].grid, h->lev[(size_t)level].grid));
  if (which == MG_OP_P && level < h->nlevels) MG_TRY(build_small_prolong(*M, h->lev[(size_t)level - 1].grid, h->lev[(size_t)level].grid));
  if (which == MG_OP_R && h->finalized && h->nrhs == 1 && level < h->nlevels)   // (the marching restriction's records hold the values)
    MG_TRY(build_marchr(*M, h->lev[(size_t)level - 1].grid, h->lev[(size_t)level].grid));
  return MG_OK;
}

// ---- device-resident hot path ---------------------------------------------------------------------
int mg_cycle_dev_FP64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs,
                      long long x_is_zero) {
  MG_REAL_ONLY(h);
  MG_TRY(check_ready(h, n, nrhs, true));
  if (h->ghost && x_is_zero < 0) return fail(MG_ERR_UNSUPPORTED, "ghost-layer form: pass x_is_zero = 0 or 1 (the norm of x is a sum over all ranks: mg_solve_dev_FP64 takes it)");
  if (!b || !x) return fail(MG_ERR_INVALID, "null vector");
  (void)hipSetDevice(h->device);
  bool xz = (x_is_zero == 1);
  if (x_is_zero < 0) {  // norm(x)>0.0 decides (MGcycle.jl:29)
    double xn = 0.0;
    MG_TRY(norm_sync(h, x, n * nrhs, &xn));
    xz = (xn == 0.0);
  }
  if (h->ghost && nrhs != 1) MG_TRY(cycle_dev_columns(h, b, x, xz));   // (ghost-layer form: a block cycle is its columns' cycles)
  else MG_TRY(cycle_dev(h, b, x, xz));
  HIP_TRY(spin_sync(h->play->stream));
  prof_collect(h);
  return MG_OK;
}

int mg_solve_dev_FP64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs,
                      double tol, long long maxIter, long long* iters, double* resvec) {
  MG_REAL_ONLY(h);
  MG_TRY(check_ready(h, n, nrhs, true));
  if (!b || !x) return fail(MG_ERR_INVALID, "null vector");
  if (maxIter < 0) return fail(MG_ERR_INVALID, "maxIter < 0");
  (void)hipSetDevice(h->device);
  if (h->ghost && nrhs != 1 && !columns_ok(h))
    return fail(MG_ERR_UNSUPPORTED, "ghost-layer form: a block of right-hand sides needs the column-wise solve (constant-coefficient fine level with the four-stage pass, V(2,*) pointwise smoother)");
  if (columns_ok(h)) MG_TRY(solve_dev_columns(h, b, x, tol, maxIter, iters, resvec));
  else MG_TRY(solve_dev(h, b, x, tol, maxIter, iters, resvec));
  HIP_TRY(spin_sync(h->play->stream));
  prof_collect(h);
  return MG_OK;
}

int mg_spmv_dev_FP64(mg_hierarchy* h, long long level, long long which, double alpha,
                     const double* x, double beta, double* y, long long nrhs) {
  MG_REAL_ONLY(h);
  MG_TRY(need_finalized(h));
  Csr* M;
  MG_TRY(find_op(h, level, which, &M));
  if (nrhs != h->nrhs) return fail(MG_ERR_INVALID, "nrhs=%lld but the scratch is sized for %lld", nrhs, h->nrhs);
  if (!x || !y) return fail(MG_ERR_INVALID, "null vector");
  if (x == y) return fail(MG_ERR_INVALID, "x and y must not alias");
  (void)hipSetDevice(h->device);
  MG_TRY(k_spmv(h, (int)level - 1, MG_K_SPMV, *M, alpha, x, beta, y));
  HIP_TRY(spin_sync(h->play->stream));
  prof_collect(h);
  return MG_OK;
}

int mg_fused_dev_FP64(mg_hierarchy* h, long long level, long long kernel, const double* b,
                      const double* x, double* out, long long nrhs) {
  MG_REAL_ONLY(h);
  MG_TRY(need_finalized(h));
  Level* L;
  MG_TRY(find_level(h, level, &L));
  if (nrhs != h->nrhs) return fail(MG_ERR_INVALID, "nrhs=%lld but the scratch is sized for %lld", nrhs, h->nrhs);
  if (!b || !x || !out || out == x) return fail(MG_ERR_INVALID, "null vector or out aliases x");
  (void)hipSetDevice(h->device);
  if (kernel == MG_K_RESIDUAL) {
    MG_TRY(k_residual(h, (int)level - 1, L->A, b, x, out));
  } else if (kernel == MG_K_SMOOTH) {
    if (!L->relax_set) return fail(MG_ERR_STATE, "relaxPrecs[%lld] was not set", level);
    MG_TRY(k_smooth(h, (int)level - 1, L->A, L->d.p, b, x, out));
  } else {
    return fail(MG_ERR_INVALID, "kernel must be MG_K_RESIDUAL or MG_K_SMOOTH");
  }
  HIP_TRY(spin_sync(h->play->stream));
  prof_collect(h);
  return MG_OK;
}

// t = x + d.*(b - A x) and r = b - A t (optionally xn = t + d.*r and ||r||^2) in one pass over the level: the fused
// form of relax's last sweep + the residual that follows it (MGcycle.jl:129-131 + 58-60; SolveFuncs.jl:26-30).
int mg_sweep_residual_dev_FP64(mg_hierarchy* h, long long level, const double* b, const double* x, double* t, double* r,
                               double* xn, double* norm_r) {
  MG_REAL_ONLY(h);
  MG_TRY(need_finalized(h));
  if (level < 1 || level >= h->nlevels) return fail(MG_ERR_INVALID, "bad level %lld", level);
  if (!b || !x || !t) return fail(MG_ERR_INVALID, "null vector");
  (void)hipSetDevice(h->device);
  if (!march2_ok(h, (int)level - 1, x, t, r, xn))
    return fail(MG_ERR_UNSUPPORTED, "level %lld is not served by the two-stage marching kernel (one right-hand side, pointwise "
                "smoother, grid operator without exception rows, distinct 16-byte aligned buffers)", level);
  MG_TRY(k_smooth_residual(h, (int)level - 1, b, x, t, r, xn, norm_r != nullptr));
  if (norm_r) MG_TRY(scalar_sync(h, norm_r));
  HIP_TRY(spin_sync(h->play->stream));
  prof_collect(h);
  return MG_OK;
}

int mg_four_stage_dev_FP64(mg_hierarchy* h, long long level, const double* b, const double* x, double* tp, double* rp,
                           double* norm_r) {
  MG_REAL_ONLY(h);
  MG_TRY(need_finalized(h));
  if (level < 1 || level >= h->nlevels) return fail(MG_ERR_INVALID, "bad level %lld", level);
  if (!b || !x || !tp || !rp) return fail(MG_ERR_INVALID, "null vector");
  (void)hipSetDevice(h->device);
  if (!march4_ok(h, (int)level - 1, x, tp, rp))
    return fail(MG_ERR_UNSUPPORTED, "level %lld is not served by the four-stage pass (one right-hand side, pointwise smoother, two "
                "pre-smoothing sweeps, z-star grid operator without exception rows, distinct 16-byte aligned buffers)", level);
  MG_TRY(k_four_stage(h, (int)level - 1, b, x, tp, rp));
  if (norm_r) MG_TRY(scalar_sync(h, norm_r));
  HIP_TRY(spin_sync(h->play->stream));
  prof_collect(h);
  return MG_OK;
}
// transposeHierarchy (MGsetup.jl:274-318) on the resident hierarchy: As[l] <- As[l]' on every level, Ps[l] <- Rs[l]' (the reference
// assigns `Ps[l] = sparse(Rs[l]'); Rs[l] = sparse(Ps[l]')` - the second line reads the NEW Ps[l], so Rs[l] keeps its values),
// relaxPrecs unchanged (conj of real numbers), the coarsest solve for the transposed operator.  The transposes are computed in
// HBM (transpose_count / _fill / _sort: deterministic stored-order CSR); the device formats are then rebuilt by the upload path
// from the transposed arrays (row classes, patterns, tile geometries are functions of the operator), mg_finalize included.
// MG_ERR_UNSUPPORTED (nothing changed) for hierarchies whose coarsest solve is held as sparse factors - the caller re-uploads.
namespace {
int transpose_on_device(const Csr& M, std::vector<long long>* colptr1, std::vector<long long>* rowval1, std::vector<double>* nzval) {
  const long long n = M.n_rows, m = M.n_cols, nnz = M.nnz;
  if (M.wide) return fail(MG_ERR_UNSUPPORTED, "operators with 64-bit row pointers (>= 2^31 non-zeros) are not transposed on the device: re-upload the transposed hierarchy");
  DevBuf<int> cnt, cursor, tcol;
  DevBuf<double> tval;
  MG_TRY(cnt.alloc((size_t)m + 1));
  MG_TRY(cursor.alloc((size_t)m));
  MG_TRY(tcol.alloc((size_t)std::max<long long>(nnz, 1)));
  MG_TRY(tval.alloc((size_t)std::max<long long>(nnz, 1)));
  HIP_TRY(hipMemset(cnt.p, 0, cnt.bytes()));
  HIP_TRY(hipMemset(cursor.p, 0, cursor.bytes()));
  const unsigned gb = (unsigned)std::min<long long>(65535, std::max<long long>(1, (nnz + mgk::BLK - 1) / mgk::BLK));
  hipLaunchKernelGGL(mgk::transpose_count, dim3(gb), dim3(mgk::BLK), 0, nullptr, M.colidx.p, nnz, cnt.p);
  HIP_TRY(hipGetLastError());
  std::vector<int> tp((size_t)m + 1);
  HIP_TRY(hipMemcpy(tp.data(), cnt.p, tp.size() * sizeof(int), hipMemcpyDeviceToHost));
  int longest = 0;
  for (long long j = 0; j < m; ++j) {
    longest = std::max(longest, tp[(size_t)j + 1]);
    tp[(size_t)j + 1] += tp[(size_t)j];
  }
  if (longest > 4096) return fail(MG_ERR_UNSUPPORTED, "a column of %d entries: the per-column sort of the device transpose is quadratic", longest);
  HIP_TRY(hipMemcpy(cnt.p, tp.data(), tp.size() * sizeof(int), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(mgk::transpose_fill, dim3((unsigned)((n + mgk::BLK - 1) / mgk::BLK)), dim3(mgk::BLK), 0, nullptr, M.rowptr.p, M.colidx.p,
                     M.val.p, (int)n, cnt.p, cursor.p, tcol.p, tval.p);
  hipLaunchKernelGGL(mgk::transpose_sort, dim3((unsigned)((m + mgk::BLK - 1) / mgk::BLK)), dim3(mgk::BLK), 0, nullptr, cnt.p, (int)m, tcol.p, tval.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  std::vector<int> tc((size_t)std::max<long long>(nnz, 1));
  nzval->resize((size_t)std::max<long long>(nnz, 1));
  HIP_TRY(hipMemcpy(tc.data(), tcol.p, (size_t)nnz * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(nzval->data(), tval.p, (size_t)nnz * sizeof(double), hipMemcpyDeviceToHost));
  colptr1->resize((size_t)m + 1);
  rowval1->resize((size_t)std::max<long long>(nnz, 1));
  for (long long j = 0; j <= m; ++j) (*colptr1)[(size_t)j] = (long long)tp[(size_t)j] + 1;
  for (long long k = 0; k < nnz; ++k) (*rowval1)[(size_t)k] = (long long)tc[(size_t)k] + 1;
  return MG_OK;
}
// the per-column sort of transpose_on_device is quadratic in the column length: refuse long columns up front
int transpose_longest_column_ok(const Csr& M) {
  const long long m = M.n_cols, nnz = M.nnz;
  DevBuf<int> cnt;
  MG_TRY(cnt.alloc((size_t)m + 1));
  HIP_TRY(hipMemset(cnt.p, 0, cnt.bytes()));
  const unsigned gb = (unsigned)std::min<long long>(65535, std::max<long long>(1, (nnz + mgk::BLK - 1) / mgk::BLK));
  hipLaunchKernelGGL(mgk::transpose_count, dim3(gb), dim3(mgk::BLK), 0, nullptr, M.colidx.p, nnz, cnt.p);
  HIP_TRY(hipGetLastError());
  std::vector<int> tp((size_t)m + 1);
  HIP_TRY(hipMemcpy(tp.data(), cnt.p, tp.size() * sizeof(int), hipMemcpyDeviceToHost));
  cnt.release();
  int longest = 0;
  for (long long j = 0; j < m; ++j) longest = std::max(longest, tp[(size_t)j + 1]);
  if (longest > 4096) return fail(MG_ERR_UNSUPPORTED, "a column of %d entries: the per-column sort of the device transpose is quadratic", longest);
  return MG_OK;
}
}  // namespace
int mg_transpose_hierarchy(mg_hierarchy* h) {
  MG_CF64_UNSUPPORTED(h);
  UploadFence upload_fence;
  MG_TRY(need_finalized(h));
  if (h->ghost) return fail(MG_ERR_UNSUPPORTED, "a rank's part of a sharded hierarchy is transposed on the host (every rank re-uploads its part)");
  if (h->coarse_lu) return fail(MG_ERR_UNSUPPORTED, "the coarsest solve is held as sparse factors: re-upload the transposed hierarchy");
  if (h->coarse_dd) return fail(MG_ERR_UNSUPPORTED, "the coarsest solve is a Schwarz sweep (mg_set_coarse_dd): set the transposed hierarchy up again");
  (void)hipSetDevice(h->device);
  graphs_clear(h);
  HIP_TRY(spin_sync(h->play->stream));
  const int nl = (int)h->nlevels;
  std::vector<long long> cp, rv;
  std::vector<double> nz;
  // every check that can refuse the call runs BEFORE the first operator is replaced ("nothing changed" holds for MG_ERR_UNSUPPORTED)
  for (int l = 0; l < nl; ++l) {
    Level& L = h->lev[(size_t)l];
    MG_TRY(transpose_longest_column_ok(L.A));
    if (l + 1 < nl) MG_TRY(transpose_longest_column_ok(L.R));
  }
  // from here on a failure (allocation, HIP) leaves a partly transposed hierarchy: the handle is marked unfinalized first, so
  // that every entry point refuses it until the caller has re-uploaded (the header says so)
  h->finalized = false;
  for (int l = 0; l < nl; ++l) {
    Level& L = h->lev[(size_t)l];
    MG_TRY(transpose_on_device(L.A, &cp, &rv, &nz));
    const long long nr = L.A.n_cols, nc = L.A.n_rows;
    MG_TRY(upload_csr(&L.A, h->opt, nr, nc, cp.data(), rv.data(), nz.data()));
    if (l + 1 < nl) {   // Ps[l] <- Rs[l]'
      MG_TRY(transpose_on_device(L.R, &cp, &rv, &nz));
      const long long pr = L.R.n_cols, pc = L.R.n_rows;
      MG_TRY(upload_csr(&L.P, h->opt, pr, pc, cp.data(), rv.data(), nz.data()));
    }
  }
  if (!h->coarse_gmres && h->Ainv.p) {   // (A')^-1 = (A^-1)'
    const long long n = h->n_coarse;
    hipLaunchKernelGGL(mgk::dense_transpose_inplace, dim3((unsigned)((n * n + mgk::BLK - 1) / mgk::BLK)), dim3(mgk::BLK), 0, nullptr, h->Ainv.p, (int)n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
  }
  h->finalized = false;
  return mg_finalize(h);
}

int mg_operator_shape(mg_hierarchy* h, long long level, long long which, long long* shape) {
  MG_REAL_ONLY(h);
  if (!h || !shape) return fail(MG_ERR_INVALID, "null argument");
  Csr* M;
  MG_TRY(find_op(h, level, which, &M));
  shape[0] = M->n_rows;
  shape[1] = M->n_cols;
  shape[2] = M->nnz;
  return MG_OK;
}
int mg_four_stage_form(mg_hierarchy* h, long long level, long long* yes, long long* geometry) {
  MG_REAL_ONLY(h);
  if (!h || !yes || !geometry) return fail(MG_ERR_INVALID, "null argument");
  Level* L;
  MG_TRY(find_level(h, level, &L));
  const Csr& A = L->A;
  *yes = (A.rc_march4 && !h->opt.no_march4) ? 1 : 0;
  for (int i = 0; i < 12; ++i) geometry[i] = 0;
  if (A.rc_march4) {
    const long long g[12] = {A.rm4.tiles_x, A.rm4.tiles_y, A.rm4.TX, A.rm4.TY, A.rm4_k1, A.rm4.nblocks, (long long)A.rm4_lds,
                             (long long)(A.rm4_fill * 100.0), A.rm4_nt, A.rm4.segs, A.rm4.seglen, A.rm4.ntab};
    for (int i = 0; i < 12; ++i) geometry[i] = g[i];
  }
  return MG_OK;
}

// ---- host-buffer hot path (what the Julia glue ccalls) ------------------------------------------
int mg_cycle_FP64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs,
                  long long x_is_zero) {
  MG_REAL_ONLY(h);
  MG_TRY(check_ready(h, n, nrhs));
  if (!b || !x) return fail(MG_ERR_INVALID, "null vector");
  (void)hipSetDevice(h->device);
  bool xz = (x_is_zero == 1);
  if (x_is_zero < 0) xz = host_all_zero(x, n * nrhs);   // norm(x) > 0.0 decides (MGcycle.jl:29)
  return staged(h, b, x, n, nrhs, xz ? StageX::skip : StageX::upload,
                [&](const double* sb, double* sx) { return cycle_dev(h, sb, sx, xz); });
}

int mg_solve_FP64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs,
                  double tol, long long maxIter, long long* iters, double* resvec) {
  MG_REAL_ONLY(h);
  MG_TRY(check_ready(h, n, nrhs));
  if (!b || !x) return fail(MG_ERR_INVALID, "null vector");
  if (maxIter < 0) return fail(MG_ERR_INVALID, "maxIter < 0");
  (void)hipSetDevice(h->device);
  return staged(h, b, x, n, nrhs, StageX::or_zero, [&](const double* sb, double* sx) {
    return columns_ok(h) ? solve_dev_columns(h, sb, sx, tol, maxIter, iters, resvec) : solve_dev(h, sb, sx, tol, maxIter, iters, resvec);
  });
}

// ---- Krylov drivers: host (column-major n x nrhs, staged) and device-resident (row-major [n][nrhs]) forms ---------------
int mg_pcg_dev_FP64(mg_hierarchy* h, const double* b, double* x, long long n, double tol,
                    long long maxIter, long long* iters, long long* flag, double* resvec) {
  MG_CF64_UNSUPPORTED(h);
  return krylov(h, b, x, n, 1, maxIter, /*device_form=*/true,
                [&](const double* bv, double* xv) { return pcg_dev(h, bv, xv, tol, maxIter, iters, flag, resvec); });
}

int mg_pcg_FP64(mg_hierarchy* h, const double* b, double* x, long long n, double tol, long long maxIter,
                long long* iters, long long* flag, double* resvec) {
  MG_CF64_UNSUPPORTED(h);
  return krylov(h, b, x, n, 1, maxIter, /*device_form=*/false,
                [&](const double* bv, double* xv) { return pcg_dev(h, bv, xv, tol, maxIter, iters, flag, resvec); });
}

int mg_fgmres_FP64(mg_hierarchy* h, const double* b, double* x, long long n, long long inner, double tol,
                   long long maxIter, long long* iters, long long* flag, double* resvec, long long* nres) {
  MG_CF64_UNSUPPORTED(h);
  return krylov(h, b, x, n, 1, maxIter, /*device_form=*/false,
                [&](const double* bv, double* xv) { return fgmres_dev(h, bv, xv, inner, tol, maxIter, iters, flag, resvec, nres); });
}

int mg_fgmres_dev_FP64(mg_hierarchy* h, const double* b, double* x, long long n, long long inner, double tol,
                       long long maxIter, long long* iters, long long* flag, double* resvec, long long* nres) {
  MG_CF64_UNSUPPORTED(h);
  return krylov(h, b, x, n, 1, maxIter, /*device_form=*/true,
                [&](const double* bv, double* xv) { return fgmres_dev(h, bv, xv, inner, tol, maxIter, iters, flag, resvec, nres); });
}

int mg_bicgstab_dev_FP64(mg_hierarchy* h, const double* b, double* x, long long n, double tol,
                         long long maxIter, long long* iters, long long* flag, double* resvec, long long* nres) {
  MG_CF64_UNSUPPORTED(h);
  return krylov(h, b, x, n, 1, maxIter, /*device_form=*/true,
                [&](const double* bv, double* xv) { return bicgstab_dev(h, bv, xv, tol, maxIter, iters, flag, resvec, nres); });
}

int mg_bicgstab_FP64(mg_hierarchy* h, const double* b, double* x, long long n, double tol, long long maxIter,
                     long long* iters, long long* flag, double* resvec, long long* nres) {
  MG_CF64_UNSUPPORTED(h);
  return krylov(h, b, x, n, 1, maxIter, /*device_form=*/false,
                [&](const double* bv, double* xv) { return bicgstab_dev(h, bv, xv, tol, maxIter, iters, flag, resvec, nres); });
}

int mg_block_pcg_dev_FP64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs, double tol,
                          long long maxIter, long long* iters, long long* flag, double* resmat) {
  MG_CF64_UNSUPPORTED(h);
  return krylov(h, b, x, n, nrhs, maxIter, /*device_form=*/true,
                [&](const double* bv, double* xv) { return block_pcg_dev(h, bv, xv, tol, maxIter, iters, flag, resmat); });
}
int mg_block_pcg_FP64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs, double tol,
                      long long maxIter, long long* iters, long long* flag, double* resmat) {
  MG_CF64_UNSUPPORTED(h);
  return krylov(h, b, x, n, nrhs, maxIter, /*device_form=*/false,
                [&](const double* bv, double* xv) { return block_pcg_dev(h, bv, xv, tol, maxIter, iters, flag, resmat); });
}
int mg_block_bicgstab_dev_FP64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs, double tol,
                               long long maxIter, long long* iters, long long* flag, double* resvec, long long* nres) {
  MG_CF64_UNSUPPORTED(h);
  return krylov(h, b, x, n, nrhs, maxIter, /*device_form=*/true,
                [&](const double* bv, double* xv) { return block_bicgstab_dev(h, bv, xv, tol, maxIter, iters, flag, resvec, nres); });
}
int mg_block_bicgstab_FP64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs, double tol,
                           long long maxIter, long long* iters, long long* flag, double* resvec, long long* nres) {
  MG_CF64_UNSUPPORTED(h);
  return krylov(h, b, x, n, nrhs, maxIter, /*device_form=*/false,
                [&](const double* bv, double* xv) { return block_bicgstab_dev(h, bv, xv, tol, maxIter, iters, flag, resvec, nres); });
}
int mg_block_fgmres_dev_FP64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs, long long inner,
                             double tol, long long maxIter, long long* iters, long long* flag, double* resvec,
                             long long* nres) {
  MG_CF64_UNSUPPORTED(h);
  return krylov(h, b, x, n, nrhs, maxIter, /*device_form=*/true,
                [&](const double* bv, double* xv) { return block_fgmres_dev(h, bv, xv, inner, tol, maxIter, iters, flag, resvec, nres); });
}
int mg_block_fgmres_FP64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs, long long inner,
                         double tol, long long maxIter, long long* iters, long long* flag, double* resvec,
                         long long* nres) {
  MG_CF64_UNSUPPORTED(h);
  return krylov(h, b, x, n, nrhs, maxIter, /*device_form=*/false,
                [&](const double* bv, double* xv) { return block_fgmres_dev(h, bv, xv, inner, tol, maxIter, iters, flag, resvec, nres); });
}

// ---- the real drivers' passes on their own: each entry runs ONE helper of the drivers above (mg_krylov.inc, mg_schedule.inc, mg_launch.inc)
// on the caller's device vectors - the drivers' grids, partial buffers and stream, n of the caller's choosing ----------------------------
int mg_kry_dot_dev_FP64(mg_hierarchy* h, const double* x, const double* y, long long n, double* out) {
  MG_TRY(kry_pass_ready(h, n, __func__));
  if (!x || !y || !out) return fail(MG_ERR_INVALID, "%s: null vector", __func__);
  return dot_sync(h, x, y, n, out);
}
int mg_kry_norm_dev_FP64(mg_hierarchy* h, const double* x, long long n, double* out) {
  MG_TRY(kry_pass_ready(h, n, __func__));
  if (!x || !out) return fail(MG_ERR_INVALID, "%s: null vector", __func__);
  return norm_sync(h, x, n, out);
}
int mg_kry_axpby_dev_FP64(mg_hierarchy* h, double a, const double* x, double b, double* y, long long n) {
  MG_TRY(kry_pass_ready(h, n, __func__));
  if (!x || !y) return fail(MG_ERR_INVALID, "%s: null vector", __func__);
  return k_axpby(h, a, x, b, y, n);
}
int mg_kry_cg_update_dev_FP64(mg_hierarchy* h, double alpha, const double* p, const double* Ap, double* x, double* r, long long n,
                              double* rnorm) {
  MG_TRY(kry_pass_ready(h, n, __func__));
  if (!p || !Ap || !x || !r) return fail(MG_ERR_INVALID, "%s: null vector", __func__);
  return rnorm ? cg_update_norm(h, alpha, p, Ap, x, r, n, rnorm) : cg_update(h, alpha, p, Ap, x, r, n);
}
int mg_kry_cg_p_dev_FP64(mg_hierarchy* h, double beta, const double* z, double* p, long long n) {
  MG_TRY(kry_pass_ready(h, n, __func__));
  if (!z || !p) return fail(MG_ERR_INVALID, "%s: null vector", __func__);
  return cg_direction(h, beta, z, p, n);
}
int mg_kry_mgs_step_dev_FP64(mg_hierarchy* h, const double* hk, const double* v, double* w, const double* u, long long n, double* out) {
  MG_TRY(kry_pass_ready(h, n, __func__));
  if (!hk || !v || !w || !out) return fail(MG_ERR_INVALID, "%s: null vector", __func__);
  mgs_update(h, hk, v, w, u, n, out);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
int mg_kry_mgs_chain_dev_FP64(mg_hierarchy* h, double* V, long long n, long long i, double* h_host) {
  MG_TRY(kry_pass_ready(h, n, __func__));
  if (!V || !h_host) return fail(MG_ERR_INVALID, "%s: null vector", __func__);
  if (i < 0 || i > 63) return fail(MG_ERR_INVALID, "%s: i=%lld outside 0..63", __func__, i);
  MG_TRY(mgs_chain(h, V, n, (int)i, (size_t)i + 2));
  std::memcpy(h_host, h->h_kscal, sizeof(double) * (size_t)(i + 2));
  return MG_OK;
}
int mg_kry_blk_gram_dev_FP64(mg_hierarchy* h, const double* X, const double* Y, long long n, long long k, double* G_host) {
  MG_TRY(kry_pass_ready(h, n, __func__));
  if (!X || !Y || !G_host) return fail(MG_ERR_INVALID, "%s: null block", __func__);
  if (k < 1 || k > mgk::BLK_KMAX) return fail(MG_ERR_INVALID, "%s: k=%lld outside 1..%d", __func__, k, mgk::BLK_KMAX);
  SmallMat G;
  MG_TRY(blk_gram(h, X, Y, n, (int)k, G));
  std::memcpy(G_host, G.a.data(), sizeof(double) * (size_t)(k * k));
  return MG_OK;
}
int mg_kry_blk_comb_dev_FP64(mg_hierarchy* h, double* out, const double* add, double s, const double* in, const double* C_host,
                             long long n, long long k) {
  MG_TRY(kry_pass_ready(h, n, __func__));
  if (!out || !in || !C_host) return fail(MG_ERR_INVALID, "%s: null block", __func__);
  if (k < 1 || k > mgk::BLK_KMAX) return fail(MG_ERR_INVALID, "%s: k=%lld outside 1..%d", __func__, k, mgk::BLK_KMAX);
  SmallMat Cm((int)k, (int)k);
  std::memcpy(Cm.a.data(), C_host, sizeof(double) * (size_t)(k * k));
  return blk_comb(h, out, add, s, in, Cm, n, (int)k);
}

// Mixed-precision preconditioner hook (getMultigridPreconditioner, SolveFuncs.jl:52-58): the caller's block is Float32,
// the hierarchy Float64: bl .= b ; z .= 0 ; recursiveCycle(param, bl, z, 1) ; z2 .= z.  b32 / z32: n x nrhs column-major.
int mg_cycle_mixed_FP32(mg_hierarchy* h, const float* b32, float* z32, long long n, long long nrhs) {
  MG_REAL_ONLY(h);
  MG_TRY(check_ready(h, n, nrhs));
  if (!b32 || !z32) return fail(MG_ERR_INVALID, "null vector");
  (void)hipSetDevice(h->device);
  const long long len = n * nrhs;
  float* f32 = reinterpret_cast<float*>(h->stage_t.p);              // n*nrhs doubles of scratch hold n*nrhs floats twice over
  HIP_TRY(hipMemcpyAsync(f32, b32, sizeof(float) * (size_t)len, hipMemcpyHostToDevice, h->play->stream));
  if (nrhs == 1) {
    hipLaunchKernelGGL(mgk::f32_to_f64, dim3(grid_for(len)), dim3(mgk::BLK), 0, h->play->stream, f32, h->stage_b.p, len);
  } else {   // column-major float -> row-major double through stage_x
    hipLaunchKernelGGL(mgk::f32_to_f64, dim3(grid_for(len)), dim3(mgk::BLK), 0, h->play->stream, f32, h->stage_x.p, len);
    hipLaunchKernelGGL(mgk::colmajor_to_rowmajor, dim3(grid_for(len)), dim3(mgk::BLK), 0, h->play->stream, h->stage_x.p, h->stage_b.p, n, (int)nrhs);
  }
  HIP_TRY(hipGetLastError());
  MG_TRY(cycle_dev(h, h->stage_b.p, h->stage_x.p, true));
  if (nrhs == 1) {
    hipLaunchKernelGGL(mgk::f64_to_f32, dim3(grid_for(len)), dim3(mgk::BLK), 0, h->play->stream, h->stage_x.p, f32, len);
  } else {
    hipLaunchKernelGGL(mgk::rowmajor_to_colmajor, dim3(grid_for(len)), dim3(mgk::BLK), 0, h->play->stream, h->stage_x.p, h->stage_b.p, n, (int)nrhs);
    hipLaunchKernelGGL(mgk::f64_to_f32, dim3(grid_for(len)), dim3(mgk::BLK), 0, h->play->stream, h->stage_b.p, f32, len);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(z32, f32, sizeof(float) * (size_t)len, hipMemcpyDeviceToHost, h->play->stream));
  HIP_TRY(spin_sync(h->play->stream));
  prof_collect(h);
  return MG_OK;
}

// Page-lock a long-lived host array (param.memCycle[1].x, the caller's b) so that the host-pointer entry points move it
// at full PCIe rate: the CALLER owns the lifetime - unregister before the array is freed or resized.
// ---- stand-alone sparse-factor applier: the device counterpart of the reference's parallelJuliaSolver backend 3 --------
// applyLUsolve_FP64_INT64 (deps/src/parLU.cpp:52-63): x[q] = U \ (L \ b[p]) (l.120-190) and, with doTranspose, the
// solve with the transposed matrix x[p] = L' \ (U' \ b[q]) (l.194-260), one right-hand side per OpenMP task there.
// Here: the factors live in HBM in the form of the coarsest solve (level-scheduled, chip-wide for large factors); the
// transposed solve uses the transposed factors (U' is lower triangular with its diagonal last, L' upper with its
// diagonal first, the permutations swap roles), built on first use.
struct mg_lu {
  int device = 0;
  long long n = 0;
  std::vector<long long> Lptr, Lcol, Uptr, Ucol, p, q;
  std::vector<double> Lval, Uval;
  mg_hierarchy* fwd = nullptr;
  mg_hierarchy* trans = nullptr;
  // value type of the factors: 0 Float64 (the hierarchies above), 1 ComplexF64, 2 Float32, 3 ComplexF32 - the last three are held by
  // the applier of mg_complex.inc in its instantiation for that type, and nothing above is used
  int kind = 0;
  CxLu* cx = nullptr;
  CxLuT<cf_t>* cf = nullptr;
  CxLuT<float>* sf = nullptr;
};
extern "C++" {   // (templates: this file sits inside the extern "C" block of the entry points)
namespace {
const char* lu_kind_name(int kind) { return kind == 0 ? "Float64" : kind == 1 ? "ComplexF64" : kind == 2 ? "Float32" : "ComplexF32"; }
template <typename V> CxLuT<V>*& mg_lu_slot(mg_lu* f);
template <> CxLuT<cx_t>*& mg_lu_slot<cx_t>(mg_lu* f) { return f->cx; }
template <> CxLuT<cf_t>*& mg_lu_slot<cf_t>(mg_lu* f) { return f->cf; }
template <> CxLuT<float>*& mg_lu_slot<float>(mg_lu* f) { return f->sf; }
}  // namespace
}  // extern "C++"
namespace {
// CSR (1-based) of the transpose of an n x n CSR (1-based) matrix; columns of every row come out ascending
void transpose_csr1(long long n, const std::vector<long long>& ptr, const std::vector<long long>& col, const std::vector<double>& val,
                    std::vector<long long>& tp, std::vector<long long>& tc, std::vector<double>& tv) {
  const size_t nnz = col.size();
  tp.assign((size_t)n + 1, 0);
  tc.resize(nnz);
  tv.resize(nnz);
  for (size_t k = 0; k < nnz; ++k) tp[(size_t)col[k]]++;            // count of column c at index c (1-based) -> shifted prefix
  long long run = 1;
  for (long long c = 0; c < n; ++c) {
    const long long cnt = tp[(size_t)c + 1];
    tp[(size_t)c] = run;
    run += cnt;
  }
  tp[(size_t)n] = run;
  std::vector<long long> pos(tp.begin(), tp.end() - 1);
  for (long long r = 0; r < n; ++r)
    for (long long k = ptr[(size_t)r] - 1; k < ptr[(size_t)r + 1] - 1; ++k) {
      const long long c = col[(size_t)k] - 1;
      const long long w = pos[(size_t)c]++ - 1;
      tc[(size_t)w] = r + 1;
      tv[(size_t)w] = val[(size_t)k];
    }
}
int lu_hierarchy(mg_lu* f, bool transposed, mg_hierarchy** out) {
  mg_hierarchy*& h = transposed ? f->trans : f->fwd;
  if (!h) {
    MG_TRY(mg_create(1, 1, f->device, &h));
    h->lu_only = true;
    int rc;
    if (!transposed) {
      rc = mg_set_coarse_lu_FP64_INT64(h, f->n, f->Lptr.data(), f->Lcol.data(), f->Lval.data(), f->Uptr.data(), f->Ucol.data(),
                                       f->Uval.data(), f->p.data(), f->q.data());
    } else {
      std::vector<long long> lp, lc, up, uc;
      std::vector<double> lv, uv;
      transpose_csr1(f->n, f->Uptr, f->Ucol, f->Uval, lp, lc, lv);   // U' : lower triangular, diagonal last
      transpose_csr1(f->n, f->Lptr, f->Lcol, f->Lval, up, uc, uv);   // L' : upper triangular, diagonal first
      rc = mg_set_coarse_lu_FP64_INT64(h, f->n, lp.data(), lc.data(), lv.data(), up.data(), uc.data(), uv.data(), f->q.data(),
                                       f->p.data());
    }
    if (rc == MG_OK) rc = mg_finalize(h);
    if (rc != MG_OK) {
      mg_destroy(h);
      h = nullptr;
      return rc;
    }
  }
  *out = h;
  return MG_OK;
}
}  // namespace

int mg_lu_create_FP64_INT64(long long device_id, long long n, const long long* Lptr, const long long* Lcol, const double* Lval,
                            const long long* Uptr, const long long* Ucol, const double* Uval, const long long* p,
                            const long long* q, mg_lu** out) {
  if (!out) return fail(MG_ERR_INVALID, "out is null");
  *out = nullptr;
  if (n < 1 || !Lptr || !Lcol || !Lval || !Uptr || !Ucol || !Uval || !p || !q) return fail(MG_ERR_INVALID, "null or empty factor");
  if (Lptr[0] != 1 || Uptr[0] != 1 || Lptr[n] < 1 || Uptr[n] < 1) return fail(MG_ERR_INVALID, "row pointers must be 1-based");
  mg_lu* f = new mg_lu();
  f->device = (int)device_id;
  f->n = n;
  f->Lptr.assign(Lptr, Lptr + n + 1);
  f->Uptr.assign(Uptr, Uptr + n + 1);
  f->Lcol.assign(Lcol, Lcol + (Lptr[n] - 1));
  f->Lval.assign(Lval, Lval + (Lptr[n] - 1));
  f->Ucol.assign(Ucol, Ucol + (Uptr[n] - 1));
  f->Uval.assign(Uval, Uval + (Uptr[n] - 1));
  f->p.assign(p, p + n);
  f->q.assign(q, q + n);
  mg_hierarchy* h = nullptr;
  const int rc = lu_hierarchy(f, false, &h);   // validates and uploads the factors
  if (rc != MG_OK) {
    delete f;
    return rc;
  }
  *out = f;
  return MG_OK;
}

// b, x: host, n x nrhs column-major (a Julia Array{Float64,2} or Vector); b is NOT used as work space (the reference
// overwrites it, parLU.cpp:176)
int mg_lu_solve_FP64(mg_lu* f, const double* b, double* x, long long n, long long nrhs, long long doTranspose) {
  if (!f) return fail(MG_ERR_INVALID, "null factor handle");
  if (f->kind != 0) return fail(MG_ERR_STATE, "mg_lu_solve_FP64 on a handle of %s factors (its own solve entry points serve it)", lu_kind_name(f->kind));
  if (n != f->n) return fail(MG_ERR_INVALID, "n=%lld but the factors have order %lld", n, f->n);
  if (nrhs < 1 || !b || !x) return fail(MG_ERR_INVALID, "bad argument");
  mg_hierarchy* h = nullptr;
  MG_TRY(lu_hierarchy(f, doTranspose != 0, &h));
  MG_TRY(mg_set_nrhs(h, nrhs));
  return mg_cycle_FP64(h, b, x, n, nrhs, 1);
}

// device-resident form: b_dev, x_dev row-major [n][nrhs] in HBM
int mg_lu_solve_dev_FP64(mg_lu* f, const double* b_dev, double* x_dev, long long n, long long nrhs, long long doTranspose) {
  if (!f) return fail(MG_ERR_INVALID, "null factor handle");
  if (f->kind != 0) return fail(MG_ERR_STATE, "mg_lu_solve_dev_FP64 on a handle of %s factors (its own solve entry points serve it)", lu_kind_name(f->kind));
  if (n != f->n) return fail(MG_ERR_INVALID, "n=%lld but the factors have order %lld", n, f->n);
  if (nrhs < 1 || !b_dev || !x_dev) return fail(MG_ERR_INVALID, "bad argument");
  mg_hierarchy* h = nullptr;
  MG_TRY(lu_hierarchy(f, doTranspose != 0, &h));
  MG_TRY(mg_set_nrhs(h, nrhs));
  return mg_cycle_dev_FP64(h, b_dev, x_dev, n, nrhs, 1);
}

// ComplexF64 factors (applyLUsolve_CFP64_INT64, parLU.cpp:69-72): values, b and x interleaved (re, im).  doTranspose solves
// with the ADJOINT, x[p] = L^H \ (U^H \ b[q]) (Julia's A'), from conjugate-transposed factors built on first use.
// Single factors (applyLUsolve_FP32_UINT32, _CFP32_UINT32, _CFP32_INT64; parLU.cpp): values, b and x in float (complex: interleaved),
// column indices and permutations in the index type of the name, row pointers Int64 as in every form.  The factors are stored in
// single and every row is evaluated in double (mg_complex.hpp).  doTranspose: the transposed (complex: adjoint) factors, as above.
extern "C++" {
namespace {
template <typename V, typename IDX>
int cxlu_create_entry(long long device_id, long long n, const long long* Lptr, const IDX* Lcol, const typename lu_store<V>::scalar* Lval,
                      const long long* Uptr, const IDX* Ucol, const typename lu_store<V>::scalar* Uval, const IDX* p, const IDX* q, mg_lu** out) {
  if (!out) return fail(MG_ERR_INVALID, "out is null");
  *out = nullptr;
  if (n < 1 || !Lptr || !Lcol || !Lval || !Uptr || !Ucol || !Uval || !p || !q) return fail(MG_ERR_INVALID, "null or empty factor");
  if (Lptr[0] != 1 || Uptr[0] != 1 || Lptr[n] < 1 || Uptr[n] < 1) return fail(MG_ERR_INVALID, "row pointers must be 1-based");
  if (n >= (1LL << 31) - 1 || Lptr[n] - 1 >= (1LL << 31) || Uptr[n] - 1 >= (1LL << 31))   // (ahead of the copies below)
    return fail(MG_ERR_UNSUPPORTED, "factors exceed int32 device indices");
  // the applier takes Int64 indices: UInt32 ones are widened here, once
  std::vector<long long> lc, uc, pp, qq;
  const long long *Lc, *Uc, *P, *Q;
  if constexpr (std::is_same<IDX, long long>::value) {
    Lc = Lcol; Uc = Ucol; P = p; Q = q;
  } else {
    lc.assign(Lcol, Lcol + (Lptr[n] - 1)); uc.assign(Ucol, Ucol + (Uptr[n] - 1));
    pp.assign(p, p + n); qq.assign(q, q + n);
    Lc = lc.data(); Uc = uc.data(); P = pp.data(); Q = qq.data();
  }
  CxLuT<V>* S = nullptr;
  MG_TRY(cxlu_create<V>(device_id, n, Lptr, Lc, Lval, Uptr, Uc, Uval, P, Q, &S));
  mg_lu* f = new mg_lu();
  f->device = (int)device_id;
  f->n = n;
  f->kind = lu_store<V>::kind;
  mg_lu_slot<V>(f) = S;
  *out = f;
  return MG_OK;
}
}  // namespace
}  // extern "C++"

int mg_lu_create_CFP64_INT64(long long device_id, long long n, const long long* Lptr, const long long* Lcol, const double* Lval,
                             const long long* Uptr, const long long* Ucol, const double* Uval, const long long* p,
                             const long long* q, mg_lu** out) {
  return cxlu_create_entry<cx_t, long long>(device_id, n, Lptr, Lcol, Lval, Uptr, Ucol, Uval, p, q, out);
}
int mg_lu_create_FP32_UINT32(long long device_id, long long n, const long long* Lptr, const unsigned int* Lcol, const float* Lval,
                             const long long* Uptr, const unsigned int* Ucol, const float* Uval, const unsigned int* p,
                             const unsigned int* q, mg_lu** out) {
  return cxlu_create_entry<float, unsigned int>(device_id, n, Lptr, Lcol, Lval, Uptr, Ucol, Uval, p, q, out);
}
int mg_lu_create_CFP32_UINT32(long long device_id, long long n, const long long* Lptr, const unsigned int* Lcol, const float* Lval,
                              const long long* Uptr, const unsigned int* Ucol, const float* Uval, const unsigned int* p,
                              const unsigned int* q, mg_lu** out) {
  return cxlu_create_entry<cf_t, unsigned int>(device_id, n, Lptr, Lcol, Lval, Uptr, Ucol, Uval, p, q, out);
}
int mg_lu_create_CFP32_INT64(long long device_id, long long n, const long long* Lptr, const long long* Lcol, const float* Lval,
                             const long long* Uptr, const long long* Ucol, const float* Uval, const long long* p,
                             const long long* q, mg_lu** out) {
  return cxlu_create_entry<cf_t, long long>(device_id, n, Lptr, Lcol, Lval, Uptr, Ucol, Uval, p, q, out);
}

extern "C++" {
namespace {
const char* lu_kind_create(int kind) {
  return kind == 1 ? "mg_lu_create_CFP64_INT64" : kind == 2 ? "mg_lu_create_FP32_UINT32" : "mg_lu_create_CFP32_UINT32 / _INT64";
}
template <typename V>
int cxlu_entry(mg_lu* f, const typename lu_store<V>::scalar* b, typename lu_store<V>::scalar* x, long long n, long long nrhs,
               long long doTranspose, bool host, const char* name) {
  if (!f) return fail(MG_ERR_INVALID, "null factor handle");
  if (f->kind != lu_store<V>::kind)
    return fail(MG_ERR_STATE, "%s on a handle of %s factors (create it with %s)", name, lu_kind_name(f->kind), lu_kind_create(lu_store<V>::kind));
  if (n != f->n) return fail(MG_ERR_INVALID, "n=%lld but the factors have order %lld", n, f->n);
  if (nrhs < 1 || !b || !x) return fail(MG_ERR_INVALID, "bad argument");
  if (n * nrhs >= (1LL << 31)) return fail(MG_ERR_UNSUPPORTED, "n*nrhs=%lld exceeds int32 device indices", n * nrhs);
  CxLuT<V>* S = mg_lu_slot<V>(f);
  (void)hipSetDevice(S->device);
  CxLuSetT<V>* G = nullptr;
  MG_TRY(cxlu_set(S, doTranspose != 0, &G));
  if (host) return cxlu_solve_host(S, *G, b, x, (int)nrhs);
  MG_TRY(cxlu_solve_dev<V>(S, *G, reinterpret_cast<const V*>(b), reinterpret_cast<V*>(x), (int)nrhs));
  HIP_TRY(spin_sync(S->stream));
  return MG_OK;
}
}  // namespace
}  // extern "C++"

// b, x: host, n x nrhs column-major ComplexF64; b is NOT used as work space
int mg_lu_solve_CFP64(mg_lu* f, const double* b, double* x, long long n, long long nrhs, long long doTranspose) {
  return cxlu_entry<cx_t>(f, b, x, n, nrhs, doTranspose, true, "mg_lu_solve_CFP64");
}

// device-resident form: b_dev, x_dev row-major [n][nrhs] ComplexF64 in HBM
int mg_lu_solve_dev_CFP64(mg_lu* f, const double* b_dev, double* x_dev, long long n, long long nrhs, long long doTranspose) {
  return cxlu_entry<cx_t>(f, b_dev, x_dev, n, nrhs, doTranspose, false, "mg_lu_solve_dev_CFP64");
}

// the same pairs for Float32 and ComplexF32 handles
int mg_lu_solve_FP32(mg_lu* f, const float* b, float* x, long long n, long long nrhs, long long doTranspose) {
  return cxlu_entry<float>(f, b, x, n, nrhs, doTranspose, true, "mg_lu_solve_FP32");
}
int mg_lu_solve_dev_FP32(mg_lu* f, const float* b_dev, float* x_dev, long long n, long long nrhs, long long doTranspose) {
  return cxlu_entry<float>(f, b_dev, x_dev, n, nrhs, doTranspose, false, "mg_lu_solve_dev_FP32");
}
int mg_lu_solve_CFP32(mg_lu* f, const float* b, float* x, long long n, long long nrhs, long long doTranspose) {
  return cxlu_entry<cf_t>(f, b, x, n, nrhs, doTranspose, true, "mg_lu_solve_CFP32");
}
int mg_lu_solve_dev_CFP32(mg_lu* f, const float* b_dev, float* x_dev, long long n, long long nrhs, long long doTranspose) {
  return cxlu_entry<cf_t>(f, b_dev, x_dev, n, nrhs, doTranspose, false, "mg_lu_solve_dev_CFP32");
}

extern "C++" {
namespace {
// the three applier kinds behind one call: fn(S) with S the handle's CxLuT<V>*
template <typename FN>
int lu_with_applier(mg_lu* f, FN&& fn) {
  return f->kind == 1 ? fn(f->cx) : f->kind == 2 ? fn(f->sf) : fn(f->cf);
}
template <typename V>
int cxlu_form(CxLuT<V>* S, long long doTranspose, long long* info) {
  (void)hipSetDevice(S->device);
  CxLuSetT<V>* G = nullptr;
  MG_TRY(cxlu_set(S, doTranspose != 0, &G));
  info[0] = lu_store<V>::kind; info[1] = G->multi ? 1 : 0; info[2] = G->M;
  info[3] = G->multi ? (long long)G->Llvl_h.size() - 1 : G->nLlvl;
  info[4] = G->multi ? (long long)G->Ulvl_h.size() - 1 : G->nUlvl;
  info[5] = G->nLlvl; info[6] = G->nUlvl;
  return MG_OK;
}
// mg_lu_time_dev on an applier handle: the samples of `warmup + reps` solves on its own stream
template <typename V>
int cxlu_time_dev(CxLuT<V>* S, const void* b_dev, void* x_dev, long long nrhs, long long doTranspose, long long warmup, long long reps,
                  double* ms) {
  CxLuSetT<V>* G = nullptr;
  MG_TRY(cxlu_set(S, doTranspose != 0, &G));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = MG_OK;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) rc = fail(MG_ERR_HIP, "hipEventCreate failed");
  for (long long it = 0; it < warmup + reps && rc == MG_OK; ++it) {
    if (hipEventRecord(e0, S->stream) != hipSuccess) rc = fail(MG_ERR_HIP, "hipEventRecord failed");
    if (rc == MG_OK) rc = cxlu_solve_dev<V>(S, *G, static_cast<const V*>(b_dev), static_cast<V*>(x_dev), (int)nrhs);
    if (rc == MG_OK) {
      float t = 0.f;
      if (hipEventRecord(e1, S->stream) != hipSuccess || spin_sync(S->stream) != hipSuccess || hipEventElapsedTime(&t, e0, e1) != hipSuccess)
        rc = fail(MG_ERR_HIP, "event timing failed");
      if (it >= warmup) ms[it - warmup] = (double)t;
    }
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  return rc;
}
}  // namespace
}  // extern "C++"

// The form a handle's factors are applied in (any value type): info[0] value type (0 Float64, 1 ComplexF64, 2 Float32,
// 3 ComplexF32), [1] 1 for the chip-wide form, [2] order of the dense trailing block, [3] / [4] launched levels of L / U around it,
// [5] / [6] all dependency levels of L / U.  doTranspose selects the transposed (adjoint) set, which is built if it was not yet.
int mg_lu_form(mg_lu* f, long long doTranspose, long long* info) {
  if (!f || !info) return fail(MG_ERR_INVALID, "null argument");
  if (f->kind != 0) return lu_with_applier(f, [&](auto* S) { return cxlu_form(S, doTranspose, info); });
  mg_hierarchy* h = nullptr;
  MG_TRY(lu_hierarchy(f, doTranspose != 0, &h));
  info[0] = 0; info[1] = h->lu_multi ? 1 : 0; info[2] = h->luML;
  info[3] = h->lu_multi ? (long long)h->luLlvl_h.size() - 1 : h->nLlvl;
  info[4] = h->lu_multi ? (long long)h->luUlvl_h.size() - 1 : h->nUlvl;
  info[5] = h->nLlvl; info[6] = h->nUlvl;
  return MG_OK;
}

// Device time of one solve on device vectors (any value type - b_dev, x_dev hold the handle's; row-major [n][nrhs]): `warmup` untimed
// solves, then `reps` solves, each enqueued between two events on the handle's stream (the second is recorded BEFORE the host waits, so
// a sample is stream time - kernels and the gaps between their launches - without the host's wake-up); ms[0..reps) in milliseconds.
// The factor set of the direction is built before the first sample, whatever `warmup` is.
int mg_lu_time_dev(mg_lu* f, const double* b_dev, double* x_dev, long long n, long long nrhs, long long doTranspose,
                   long long warmup, long long reps, double* ms) {
  if (!f || !ms || !b_dev || !x_dev || reps < 1 || warmup < 0 || nrhs < 1) return fail(MG_ERR_INVALID, "bad argument");
  if (n != f->n) return fail(MG_ERR_INVALID, "n=%lld but the factors have order %lld", n, f->n);
  (void)hipSetDevice(f->device);
  if (f->kind != 0) {
    if (n * nrhs >= (1LL << 31)) return fail(MG_ERR_UNSUPPORTED, "n*nrhs=%lld exceeds int32 device indices", n * nrhs);
    return lu_with_applier(f, [&](auto* S) { return cxlu_time_dev(S, b_dev, x_dev, nrhs, doTranspose, warmup, reps, ms); });
  }
  mg_hierarchy* h = nullptr;
  MG_TRY(lu_hierarchy(f, doTranspose != 0, &h));
  MG_TRY(mg_set_nrhs(h, nrhs));
  MG_TRY(check_ready(h, n, nrhs));
  const hipStream_t stream = h->play->stream;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = MG_OK;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) rc = fail(MG_ERR_HIP, "hipEventCreate failed");
  for (long long it = 0; it < warmup + reps && rc == MG_OK; ++it) {
    if (hipEventRecord(e0, stream) != hipSuccess) rc = fail(MG_ERR_HIP, "hipEventRecord failed");
    if (rc == MG_OK) rc = cycle_dev(h, b_dev, x_dev, true);
    if (rc == MG_OK) {
      float t = 0.f;
      if (hipEventRecord(e1, stream) != hipSuccess || spin_sync(stream) != hipSuccess || hipEventElapsedTime(&t, e0, e1) != hipSuccess)
        rc = fail(MG_ERR_HIP, "event timing failed");
      if (it >= warmup) ms[it - warmup] = (double)t;
    }
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  prof_collect(h);
  return rc;
}

int mg_lu_destroy(mg_lu* f) {
  if (!f) return MG_OK;
  if (f->cx) cxlu_destroy(f->cx);
  if (f->cf) cxlu_destroy(f->cf);
  if (f->sf) cxlu_destroy(f->sf);
  if (f->fwd) mg_destroy(f->fwd);
  if (f->trans) mg_destroy(f->trans);
  delete f;
  return MG_OK;
}

int mg_host_register(void* ptr, long long bytes) {
  if (!ptr || bytes < 1) return fail(MG_ERR_INVALID, "null pointer or empty range");
  HIP_TRY(hipHostRegister(ptr, (size_t)bytes, hipHostRegisterDefault));
  return MG_OK;
}
int mg_host_unregister(void* ptr) {
  if (!ptr) return fail(MG_ERR_INVALID, "null pointer");
  HIP_TRY(hipHostUnregister(ptr));
  return MG_OK;
}

int mg_spmv_FP64(mg_hierarchy* h, long long level, long long which, double alpha, const double* x,
                 double beta, double* y, long long nrhs) {
  MG_REAL_ONLY(h);
  MG_TRY(need_finalized(h));
  Csr* M;
  MG_TRY(find_op(h, level, which, &M));
  if (nrhs != h->nrhs) return fail(MG_ERR_INVALID, "nrhs=%lld but the scratch is sized for %lld", nrhs, h->nrhs);
  if (!x || !y) return fail(MG_ERR_INVALID, "null vector");
  (void)hipSetDevice(h->device);
  MG_TRY(upload_block(h, x, h->stage_x.p, M->n_cols, nrhs));
  if (beta != 0.0) MG_TRY(upload_block(h, y, h->stage_b.p, M->n_rows, nrhs));
  MG_TRY(k_spmv(h, (int)level - 1, MG_K_SPMV, *M, alpha, h->stage_x.p, beta, h->stage_b.p));
  MG_TRY(download_block(h, h->stage_b.p, y, M->n_rows, nrhs));
  prof_collect(h);
  return MG_OK;
}

// ---- measurement --------------------------------------------------------------------------------------
int mg_time_op_dev_FP64(mg_hierarchy* h, long long level, long long kernel, long long nrhs,
                        long long reps, double* ms_avg, double* bytes) {
  MG_REAL_ONLY(h);
  MG_TRY(need_finalized(h));
  Level* Lp;
  MG_TRY(find_level(h, level, &Lp));
  if (nrhs != h->nrhs) return fail(MG_ERR_INVALID, "nrhs=%lld but the scratch is sized for %lld", nrhs, h->nrhs);
  if (reps < 1 || !ms_avg) return fail(MG_ERR_INVALID, "reps < 1 or null output");
  (void)hipSetDevice(h->device);
  const int l = (int)level - 1;
  Level& L = *Lp;
  const bool coarsest = (l == (int)h->nlevels - 1);
  if (coarsest && kernel != MG_K_COARSE && kernel != MG_K_SPMV && kernel != MG_K_RESIDUAL)
    return fail(MG_ERR_INVALID, "kernel %lld does not run on the coarsest level", kernel);
  // operands: the level's own scratch (contents are whatever the last cycle left: finite values)
  Play::Vecs& V = h->play->lev[(size_t)l];
  double* const Lr = h->play->res(l);
  const double* bvec = (l == 0) ? (h->last_b ? h->last_b : h->stage_b.p) : V.b.p;
  double* xa = (l == 0) ? (h->last_x ? h->last_x : h->stage_x.p) : V.x0.p;
  double* xb = V.x1.p;
  const bool was_prof = h->prof;
  h->prof = false;
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  double bts = 0.0;
  int rc = MG_OK;
  for (long long it = -2; it < reps && rc == MG_OK; ++it) {  // two untimed warm-up launches
    if (it == 0) (void)hipEventRecord(e0, h->play->stream);
    switch (kernel) {
      case MG_K_SPMV:
        rc = k_spmv(h, l, MG_K_SPMV, L.A, 1.0, xa, 0.0, Lr);
        bts = spmv_bytes(L.A, nrhs, false, false);
        break;
      case MG_K_RESIDUAL:
        rc = k_residual(h, l, L.A, bvec, xa, Lr);
        bts = spmv_bytes(L.A, nrhs, true, false);
        break;
      case MG_K_SMOOTH:
        rc = k_smooth(h, l, L.A, L.d.p, bvec, xa, xb);
        bts = spmv_bytes(L.A, nrhs, true, true);
        break;
      case MG_K_RESTRICT:
        rc = k_spmv(h, l, MG_K_RESTRICT, L.R, 1.0, Lr, 0.0, h->play->lev[(size_t)l + 1].b.p);
        bts = spmv_bytes(L.R, nrhs, false, false);
        break;
      case MG_K_SMOOTH_RESIDUAL:
        if (!march2_ok(h, l, xa, xb, Lr, nullptr)) rc = fail(MG_ERR_UNSUPPORTED, "level %lld is not served by the two-stage marching kernel", level);
        else rc = k_smooth_residual(h, l, bvec, xa, xb, Lr, nullptr, false);
        bts = spmv_bytes(L.A, nrhs, true, true) + spmv_bytes(L.A, nrhs, true, false);
        break;
      case MG_K_FOUR_STAGE:
        if (!march4_ok(h, l, xa, xb, Lr)) rc = fail(MG_ERR_UNSUPPORTED, "level %lld is not served by the four-stage pass", level);
        else rc = k_four_stage(h, l, bvec, xa, xb, Lr);
        bts = 2.0 * (spmv_bytes(L.A, nrhs, true, true) + spmv_bytes(L.A, nrhs, true, false));
        break;
      case MG_K_PROLONG:
        rc = k_spmv(h, l, MG_K_PROLONG, L.P, 0.0, h->play->lev[(size_t)l + 1].x0.p, 1.0, xb);
        bts = spmv_bytes(L.P, nrhs, true, false);
        break;
      case MG_K_DSCALE:
        rc = k_dscale(h, l, L.d.p, bvec, xb, L.n);
        bts = 8.0 * (double)L.n * (1.0 + 2.0 * (double)nrhs);
        break;
      case MG_K_COARSE:
        if (!coarsest) rc = fail(MG_ERR_INVALID, "MG_K_COARSE runs on the coarsest level only");
        else rc = k_coarse(h, l, V.b.p, V.x0.p);
        bts = h->coarse_lu ? 12.0 * (double)(h->luLval.n + h->luUval.n) + 16.0 * (double)L.n * (double)nrhs
                           : 8.0 * ((double)L.n * (double)L.n + 2.0 * (double)L.n * (double)nrhs);
        break;
      case MG_K_NORM:
        rc = k_sumsq(h, Lr, L.n * nrhs);
        bts = 8.0 * (double)L.n * (double)nrhs;
        break;
      default:
        rc = fail(MG_ERR_INVALID, "unknown kernel %lld", kernel);
    }
  }
  if (rc == MG_OK) {
    (void)hipEventRecord(e1, h->play->stream);
    hipError_t e = spin_sync(h->play->stream);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    if (e != hipSuccess) rc = fail(MG_ERR_HIP, "event timing failed: %s", hipGetErrorString(e));
    *ms_avg = (double)ms / (double)reps;
    if (bytes) *bytes = bts;
  }
  (void)spin_sync(h->play->stream);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  h->prof = was_prof;
  return rc;
}

int mg_profile_enable(mg_hierarchy* h, long long on) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  h->prof = (on != 0);
  return MG_OK;
}
int mg_profile_reset(mg_hierarchy* h) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  for (auto& s : h->slots) s = ProfSlot();
  return MG_OK;
}
int mg_profile_get(mg_hierarchy* h, long long level, long long kernel, double* total_ms,
                   long long* launches, double* bytes_per_launch) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  if (level < 1 || level > h->nlevels || kernel < 0 || kernel >= MG_K_COUNT)
    return fail(MG_ERR_INVALID, "bad (level=%lld, kernel=%lld)", level, kernel);
  const ProfSlot& s = h->slots[(size_t)(level - 1) * MG_K_COUNT + (size_t)kernel];
  if (total_ms) *total_ms = s.ms;
  if (launches) *launches = s.launches;
  if (bytes_per_launch) *bytes_per_launch = s.launches > 0 ? s.bytes / (double)s.launches : 0.0;
  return MG_OK;
}

int mg_profile_get_moved(mg_hierarchy* h, long long level, long long kernel, double* moved_bytes_per_launch) {
  MG_REAL_ONLY(h);
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  if (level < 1 || level > h->nlevels || kernel < 0 || kernel >= MG_K_COUNT || !moved_bytes_per_launch)
    return fail(MG_ERR_INVALID, "bad (level=%lld, kernel=%lld)", level, kernel);
  const ProfSlot& sl = h->slots[(size_t)(level - 1) * MG_K_COUNT + (size_t)kernel];
  *moved_bytes_per_launch = sl.launches > 0 ? sl.moved / (double)sl.launches : 0.0;
  return MG_OK;
}

int mg_operator_format(mg_hierarchy* h, long long level, long long which, long long* npatterns,
                       long long* dict_entries, double* index_bytes_per_launch) {
  MG_REAL_ONLY(h);
  Csr* M;
  MG_TRY(find_op(h, level, which, &M));
  if (npatterns) *npatterns = M->has_pat ? M->npat : 0;
  if (dict_entries) *dict_entries = M->has_pat ? M->dict_entries : 0;
  // bytes of row pointers + column information one nrhs=1 launch streams
  if (index_bytes_per_launch)
    *index_bytes_per_launch = M->has_pat
        ? (M->has_runs ? 20.0 * (double)M->nruns_total + 8.0 * (double)M->nblocks : 10.0 * (double)M->n_rows) +
              4.0 * (double)M->dict_entries
        : 4.0 * (double)M->nnz + 4.0 * (double)(M->n_rows + 1);
  return MG_OK;
}

int mg_operator_rowclasses(mg_hierarchy* h, long long level, long long which, long long* nclasses,
                           long long* dict_entries, double* matrix_bytes_per_launch) {
  MG_REAL_ONLY(h);
  Csr* M;
  MG_TRY(find_op(h, level, which, &M));
  if (nclasses) *nclasses = M->has_rc ? M->rc_ncls : 0;
  if (dict_entries) *dict_entries = M->has_rc ? M->rc_entries : 0;
  if (matrix_bytes_per_launch) {
    if (M->has_rc) {
      *matrix_bytes_per_launch = (M->rc_implicit ? 2.0 : 6.0) * (double)M->n_rows + 12.0 * (double)M->rc_entries;
    } else if (M->has_pat) {
      *matrix_bytes_per_launch = 8.0 * (double)M->nnz + 4.0 * (double)M->dict_entries +
          (M->has_runs ? 20.0 * (double)M->nruns_total + 8.0 * (double)M->nblocks : 10.0 * (double)M->n_rows);
    } else {
      *matrix_bytes_per_launch = 12.0 * (double)M->nnz + 4.0 * (double)(M->n_rows + 1);
    }
  }
  return MG_OK;
}

int mg_operator_rowclass_flags(mg_hierarchy* h, long long level, long long which, long long* implicit_first,
                               long long* class_relax, long long* kernel_variant, long long* exception_rows) {
  MG_REAL_ONLY(h);
  Csr* M;
  MG_TRY(find_op(h, level, which, &M));
  if (implicit_first) *implicit_first = (M->has_rc && M->rc_implicit) ? 1 : 0;
  if (class_relax) *class_relax = (M->has_rc && M->rc_has_d) ? 1 : 0;
  if (kernel_variant) {
    if (h->nrhs > 1)   // block right-hand sides: 5 csr_rowclass_lane_spmm, 6 csr_rowclass_lane_spmm2, else the CSR stream
      *kernel_variant = (M->has_rc && M->rc_lane_mm() && M->ln_blocks > 0) ? (lane_mm_pairs(*M, h->nrhs) ? 6 : 5) : -1;
    else if (which == MG_OP_R && M->waver_ok)
      *kernel_variant = 11;  // restriction of a vertex-centred grid pair, 62 coarse nodes per wavefront (grid_wave_restrict, any size)
    else if (which == MG_OP_P && M->cellp_ok)
      *kernel_variant = 10;  // prolongation of a vertex-centred grid pair, a lane per coarse cell (grid_cell_prolong, any size)
    else if ((which == MG_OP_A && M->sm_use()) || (which == MG_OP_R && M->smr_use()) || (which == MG_OP_P && M->smp_use()))
      *kernel_variant = 8;   // the one-trip kernels of the small grid levels (mg_small.hpp)
    else if (which == MG_OP_A && M->b27_ok)
      *kernel_variant = 9;   // band-27: planar values of a variable-coefficient 27-point grid operator
    else
      *kernel_variant = !M->has_rc ? -1 : (M->rc_marchr && !M->opt.no_marchr) ? 7 : M->rc_march ? 3 : M->rc_tile ? 2 : M->rc_window ? 1 : M->rc_lane() ? 4 : 0;
  }
  if (exception_rows) *exception_rows = M->has_rc ? M->rc_nexc : 0;
  return MG_OK;
}

// Which kernel serves an operator that is NOT stored as row classes / grid records (kernel_variant -1 above), as launch_csr picks it
// for the handle's nrhs.  info[0]: 0 none of these (a row-class or grid kernel serves it), 1 csr_pattern_spmv, 2 csr_stream_spmv,
// 3 csr_longrow_spmv, 4 csr_stream_spmm; 5 csr_rowclass_lane_spmm, 6 csr_rowclass_lane_spmm2 (nrhs > 1, row classes).  info[1]: the
// NT template argument (non-temporal loads of the matrix stream) of 1-4, rows per lane (2 or 3) of 6.  info[2]: 16-bit column
// offsets (kernel 3).  info[3]: longest row.  Read-only.  It MIRRORS launch_csr's choice from the operator's flags, it does not record a
// launch: the answer holds for the calls the cycle and mg_spmv_dev / mg_fused_dev make - the whole product (phase 0), y != x, no ||out||^2
// partials, and for kernel 6 vectors at 16-byte aligned addresses (otherwise launch_csr takes csr_stream_spmm).  A wide operator (64-bit row
// pointers) serves one right-hand side only: 0 for nrhs > 1.
int mg_operator_stream_kernel(mg_hierarchy* h, long long level, long long which, long long* info) {
  MG_REAL_ONLY(h);
  if (!info) return fail(MG_ERR_INVALID, "null argument");
  Csr* M;
  MG_TRY(find_op(h, level, which, &M));
  long long variant = 0;
  MG_TRY(mg_operator_rowclass_flags(h, level, which, nullptr, nullptr, &variant, nullptr));
  info[0] = info[1] = info[2] = 0;
  info[3] = M->max_row_nnz;
  if (h->nrhs > 1 && M->wide) return MG_OK;
  if (h->nrhs > 1) {
    const bool lane = M->rc_lane_mm() && M->ln_blocks > 0 && M->ln_rows == lane_mm_rpl(*M, h->nrhs) * (mgk::BLK / lane_mm_group(*M, h->nrhs));
    info[0] = lane ? (lane_mm_pairs(*M, h->nrhs) ? 6 : 5) : 4;
    info[1] = lane ? (lane_mm_pairs(*M, h->nrhs) ? lane_mm_rpl(*M, h->nrhs) : 2) : (M->nt ? 1 : 0);
  } else if (M->wide || variant == -1) {
    info[0] = M->longrow() ? 3 : (!M->wide && M->has_pat) ? 1 : 2;
    info[1] = M->nt ? 1 : 0;
    info[2] = (info[0] == 3 && !M->wide && M->has_ci16) ? 1 : 0;
  }
  return MG_OK;
}

// Which kernel fuses a sweep with the residual that follows it on this level's A (one right-hand side): *form = 0 none
// (two launches), 2 csr_rowclass_march2_spmv (1-D chunks), 3 csr_rowclass_march3_spmv (2-D in-plane tiles).  geometry
// (optional, 12 entries, form 3): tiles per line, tiles per column, TX, TY, rows of the stage-1 region per lane (K1),
// workgroups, dynamic LDS bytes, estimated bytes filled + stored per row x 100, threads per workgroup, segments of the
// lockstep schedule (0: balanced ranges), planes per segment, entries of the class table.
int mg_sweep_residual_form(mg_hierarchy* h, long long level, long long* form, long long* geometry) {
  MG_REAL_ONLY(h);
  if (!h || !form) return fail(MG_ERR_INVALID, "null argument");
  Level* L;
  MG_TRY(find_level(h, level, &L));
  const Csr& A = L->A;
  *form = 0;
  if (!A.set || h->nrhs != 1) return MG_OK;
  const bool band = A.rm3_var && A.rc_march3;
  if (!band && (!A.has_rc || !A.rc_has_d || A.rc_nexc != 0)) return MG_OK;
  if (A.rc_march3) {
    *form = band ? 4 : 3;
    if (geometry) {
      const long long g[12] = {A.rm3.tiles_x, A.rm3.tiles_y, A.rm3.TX, A.rm3.TY, A.rm3_k1, A.rm3.nblocks, (long long)A.rm3_lds,
                               (long long)(A.rm3_fill * 100.0), A.rm3_nt, A.rm3.segs, A.rm3.seglen, A.rm3.ntab};
      std::copy(g, g + 12, geometry);
    }
  } else if (A.rc_march && A.rc_march2) {
    *form = 2;
  } else if (A.rc_march27 && !A.opt.no_march27) {
    *form = 5;
    if (geometry) {   // the pair's geometry; [7] = workgroups of the single-product geometry
      const long long g[12] = {A.rm27[1].tiles_x, A.rm27[1].tiles_y, A.rm27[1].TX, A.rm27[1].TY, 1, A.rm27[1].nblocks, (long long)A.rm27_lds[1],
                               A.rm27[0].nblocks, A.rm27_nt[1], A.rm27[1].segs, A.rm27[1].seglen, A.rm27[1].ntab};
      std::copy(g, g + 12, geometry);
    }
  }
  return MG_OK;
}

int mg_band_form(mg_hierarchy* h, long long level, long long* info) {
  MG_REAL_ONLY(h);
  if (!h || !info) return fail(MG_ERR_INVALID, "null argument");
  Level* L;
  MG_TRY(find_level(h, level, &L));
  const Csr& A = L->A;
  const bool band = A.set && A.rm3_var && A.rc_march3;
  info[0] = band ? 1 : 0;
  info[1] = band && A.band_canon ? 1 : 0;
  info[2] = band && A.band_sym ? 1 : 0;
  info[3] = band ? (A.band_sym ? 4 : 7) : 0;
  if (!band && A.set && A.b27_ok) {     // band-27 (27 planar arrays, always in canonical slots)
    info[0] = 2;
    info[1] = 1;
    info[2] = A.b27.sym;
    info[3] = A.b27.sym ? 14 : 27;
  }
  return MG_OK;
}

int mg_cycle_bytes(mg_hierarchy* h, double* bytes) {
  MG_REAL_ONLY(h);
  if (!h || !bytes) return fail(MG_ERR_INVALID, "null argument");
  if (!h->finalized) return fail(MG_ERR_STATE, "hierarchy not finalized");
  // one V-cycle from x = 0 (SURVEY.md 8d "minimal-traffic fused model"); W/F revisit coarse levels
  // and are accounted by the profile counters instead.
  const long long k = h->nrhs;
  double t = 0.0;
  const int nl = (int)h->nlevels;
  for (int l = 0; l < nl - 1; ++l) {
    const Level& L = h->lev[(size_t)l];
    const long long npre = std::max<long long>(1, L.npre), npost = std::max<long long>(1, L.npost);
    t += 8.0 * (double)L.n * (1.0 + 2.0 * (double)k);                          // x = d.*b
    t += (double)(npre - 1 + npost) * spmv_bytes(L.A, k, true, true);          // fused sweeps
    t += spmv_bytes(L.A, k, true, false);                                      // residual
    t += spmv_bytes(L.R, k, false, false);                                     // restriction
    t += spmv_bytes(L.P, k, true, false);                                      // prolongation-add
  }
  const double nc = (double)h->n_coarse;
  t += 8.0 * (nc * nc + 2.0 * nc * (double)k);
  *bytes = t;
  return MG_OK;
}

int mg_device_bytes(mg_hierarchy* h, double* bytes) {
  MG_REAL_ONLY(h);
  if (!h || !bytes) return fail(MG_ERR_INVALID, "null argument");
  double t = 0.0;
  for (auto& L : h->lev) t += (double)(L.A.bytes() + L.P.bytes() + L.R.bytes() + L.d.bytes());
  for (auto& V : h->lane0.lev) t += (double)(V.b.bytes() + V.r.bytes() + V.x0.bytes() + V.x1.bytes());
  t += (double)(h->Ainv.bytes() + h->stage_b.bytes() + h->stage_x.bytes() + h->stage_t.bytes());
  *bytes = t;
  return MG_OK;
}

// ---- stand-alone operators and vector kernels (building blocks of the multi-GPU cycle) ------------
struct mg_operator {
  int device = 0;
  Csr M;
  DevBuf<double> m3sink, m3scratch;   // csr_rowclass_march3_spmv: store sink; outputs nobody asked for
};

int mg_op_create_FP64_INT64(long long device_id, long long n_rows, long long n_cols,
                            const long long* colptr, const long long* rowval, const double* nzval,
                            mg_operator** out) {
  UploadFence upload_fence;
  if (!out) return fail(MG_ERR_INVALID, "out is null");
  *out = nullptr;
  MG_TRY(use_device(device_id));
  mg_operator* op = new mg_operator();
  op->device = (int)device_id;
  const int rc = upload_csr(&op->M, Options::from_env(), n_rows, n_cols, colptr, rowval, nzval);
  if (rc != MG_OK) {
    op->M.release();
    delete op;
    return rc;
  }
  *out = op;
  return MG_OK;
}

// A rank's local operator of a sharded level in BOX form: square, rows/columns [owned box in natural x-fastest order |
// halo], the halo rows empty; n1 x n2 x n3 = the owned box (= regular_cols rows).  Rows that read a halo column become
// exception rows (phase 2 of mg_op_apply_phase_dev_FP64), all others keep the row-class form of the global grid operator
// and run the staged kernels (z-marching / plane tiles) of the single-GPU path.
int mg_op_create_box_FP64_INT64(long long device_id, long long n_rows, long long n_cols, const long long* colptr,
                                const long long* rowval, const double* nzval, long long n1, long long n2, long long n3,
                                long long regular_cols, mg_operator** out) {
  UploadFence upload_fence;
  if (!out) return fail(MG_ERR_INVALID, "out is null");
  *out = nullptr;
  if (n_rows != n_cols || regular_cols < 1 || regular_cols > n_rows || n1 * n2 * n3 != regular_cols)
    return fail(MG_ERR_INVALID, "box operator must be square with n1*n2*n3 == regular_cols <= n_rows");
  MG_TRY(use_device(device_id));
  mg_operator* op = new mg_operator();
  op->device = (int)device_id;
  int rc = upload_csr(&op->M, Options::from_env(), n_rows, n_cols, colptr, rowval, nzval, regular_cols);
  const long long grid[3] = {n1, n2, n3};
  if (rc == MG_OK) rc = build_staged(op->M, grid);
  if (rc != MG_OK) {
    op->M.release();
    delete op;
    return rc;
  }
  *out = op;
  return MG_OK;
}

// A transfer operator of a sharded level with grid hints: rows = a fine box f1 x f2 x f3 (n_rows, natural order), columns =
// [owned coarse box c1 x c2 x c3 (regular_cols) | halo].  The rows that read a halo column become exception rows; the others
// take the LDS-staged prolongation kernel (csr_rowclass_winp_spmv) when the pattern fits it, with the same phase split as box
// operators: phase 1 overlaps the exchange of the coarse vector, phase 2 follows it.
int mg_op_create_grid_FP64_INT64(long long device_id, long long n_rows, long long n_cols, const long long* colptr,
                                 const long long* rowval, const double* nzval, long long regular_cols, long long f1, long long f2,
                                 long long f3, long long c1, long long c2, long long c3, mg_operator** out) {
  UploadFence upload_fence;
  if (!out) return fail(MG_ERR_INVALID, "out is null");
  *out = nullptr;
  const bool hints = f1 != 0 || f2 != 0 || f3 != 0 || c1 != 0 || c2 != 0 || c3 != 0;   // (all zero: only the owned | halo split)
  if (regular_cols < 1 || regular_cols > n_cols || (hints && (f1 * f2 * f3 != n_rows || c1 * c2 * c3 != regular_cols)))
    return fail(MG_ERR_INVALID, "grid operator: f1*f2*f3 must equal n_rows and c1*c2*c3 regular_cols <= n_cols");
  MG_TRY(use_device(device_id));
  mg_operator* op = new mg_operator();
  op->device = (int)device_id;
  int rc = upload_csr(&op->M, Options::from_env(), n_rows, n_cols, colptr, rowval, nzval, regular_cols, n_rows);
  const long long gf[3] = {f1, f2, f3}, gc[3] = {c1, c2, c3};
  if (rc == MG_OK && hints) rc = build_winp(op->M, gf, gc);
  if (rc != MG_OK) {
    op->M.release();
    delete op;
    return rc;
  }
  *out = op;
  return MG_OK;
}

int mg_op_kernel_variant(mg_operator* op, long long* variant, long long* exception_rows) {
  if (!op) return fail(MG_ERR_INVALID, "null operator");
  const Csr& M = op->M;
  if (variant) *variant = !M.has_rc ? -1 : M.rc_march ? 3 : M.rc_tile ? 2 : M.rc_window ? 1 : M.rp_ok ? 5 : M.rc_lane() ? 4 : 0;
  if (exception_rows) *exception_rows = M.has_rc ? M.rc_nexc : 0;
  return MG_OK;
}

int mg_op_destroy(mg_operator* op) {
  if (!op) return MG_OK;
  (void)hipSetDevice(op->device);
  op->M.release();
  op->m3sink.release();
  op->m3scratch.release();
  delete op;
  return MG_OK;
}

// Announce the relaxPrec vector (device, one entry per regular row) this operator will be swept with: when it is
// bit-identical over every dictionary class the fused sweeps called with THIS pointer read it from the dictionary
// instead of streaming it.  Call again after the vector's contents change.
int mg_op_bind_relax_dev_FP64(mg_operator* op, const double* d_dev, long long n) {
  UploadFence upload_fence;
  if (!op || !op->M.set || !d_dev || n < 1) return fail(MG_ERR_INVALID, "bad argument");
  (void)hipSetDevice(op->device);
  (void)hipDeviceSynchronize();   // d may have been written on another stream
  return derive_class_d_csr(op->M, d_dev, (size_t)n);
}

int mg_op_apply_dev_FP64(mg_operator* op, long long kernel, double alpha, const double* x, double beta,
                         double* y, const double* b, const double* d, long long nrhs, void* stream) {
  return mg_op_apply_rows_dev_FP64(op, kernel, alpha, x, beta, y, b, d, nrhs, 0, stream);
}

int mg_op_apply_rows_dev_FP64(mg_operator* op, long long kernel, double alpha, const double* x, double beta,
                              double* y, const double* b, const double* d, long long nrhs,
                              long long row_offset, void* stream) {
  return mg_op_apply_phase_dev_FP64(op, kernel, alpha, x, beta, y, b, d, nrhs, row_offset, 0, stream);
}

int mg_op_apply_phase_dev_FP64(mg_operator* op, long long kernel, double alpha, const double* x, double beta,
                               double* y, const double* b, const double* d, long long nrhs,
                               long long row_offset, long long phase, void* stream) {
  if (!op || !op->M.set) return fail(MG_ERR_INVALID, "null or empty operator");
  if (phase < 0 || phase > 2) return fail(MG_ERR_INVALID, "phase must be 0, 1 or 2");
  if (!x || !y || nrhs < 1 || row_offset < 0) return fail(MG_ERR_INVALID, "null vector, nrhs < 1 or negative row offset");
  if (kernel == MG_K_SMOOTH && y == x) return fail(MG_ERR_INVALID, "the Jacobi update must not alias x");
  mgk::VecArgs v{};
  v.x = x;
  v.xs = x + row_offset * nrhs;
  v.y = y + row_offset * nrhs;
  v.b = b ? b + row_offset * nrhs : nullptr;
  v.d = d ? d + row_offset : nullptr;
  v.d_full = v.d;
  // relaxPrec bound to this operator and constant per class: read from the dictionary (2 B/row instead of 10)
  if (d && nrhs == 1 && row_offset == 0 && op->M.has_rc && op->M.rc_has_d && d == op->M.d_bound) v.d = nullptr;
  v.alpha = alpha;
  v.beta = beta;
  v.nrhs = (int)nrhs;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  switch (kernel) {
    case MG_K_SPMV:
    case MG_K_RESTRICT:
    case MG_K_PROLONG:
      return launch_csr<mgk::AXPBY>(s, op->M, v, nullptr, (int)phase);
    case MG_K_RESIDUAL:
      if (!b) return fail(MG_ERR_INVALID, "residual needs b");
      return launch_csr<mgk::RESID>(s, op->M, v, nullptr, (int)phase);
    case MG_K_SMOOTH:
      if (!b || !d) return fail(MG_ERR_INVALID, "smoother needs b and d");
      return launch_csr<mgk::SMOOTH>(s, op->M, v, nullptr, (int)phase);
    default:
      return fail(MG_ERR_INVALID, "kernel %lld is not an operator kernel", kernel);
  }
}

// r = b - M x on an operator with the squared norm of r fused (per-workgroup partials written from partials_dev on,
// *nparts of them) and, optionally, xnext = x + d.*r as a second output (the next cycle's first damped-Jacobi update);
// r_dev may be NULL when only the norm and xnext are wanted.  phase as mg_op_apply_phase_dev_FP64.  One right-hand side.
int mg_op_residual_fused_dev_FP64(mg_operator* op, const double* x, const double* b, const double* d, double* r_dev,
                                  double* xnext_dev, double* partials_dev, long long phase, long long* nparts, void* stream) {
  if (!op || !op->M.set) return fail(MG_ERR_INVALID, "null or empty operator");
  if (!x || !b || !partials_dev || !nparts || phase < 0 || phase > 2 || (xnext_dev && !d)) return fail(MG_ERR_INVALID, "bad argument");
  const Csr& M = op->M;
  mgk::VecArgs v{};
  v.x = x;
  v.xs = x;
  v.y = r_dev;
  v.b = b;
  v.nrhs = 1;
  v.sumsq = partials_dev;
  // the staged row-class kernels (march, tile) and the exception-row kernel can write the second output
  const bool can_y2 = M.has_rc && (M.rc_tile || march_ok(M, v)) && xnext_dev && xnext_dev != x && !(phase == 0 && M.rc_nexc > 0);
  if (can_y2) {
    v.y2 = xnext_dev;
    v.d = (M.rc_has_d && d == M.d_bound) ? nullptr : d;
    v.d_full = d;
  } else if (!r_dev) {
    return fail(MG_ERR_INVALID, "this operator's kernel cannot produce xnext: pass r_dev");
  }
  int np = 0;
  MG_TRY(launch_csr<mgk::RESID>(reinterpret_cast<hipStream_t>(stream), M, v, &np, (int)phase));
  *nparts = np;
  return MG_OK;
}
// 1 if mg_op_residual_fused_dev_FP64 can write xnext for this operator and these vectors (x 16-byte aligned etc.)
int mg_op_can_fuse_next(mg_operator* op, const double* x, long long* yes) {
  if (!op || !yes) return fail(MG_ERR_INVALID, "null argument");
  mgk::VecArgs v{};
  v.x = x;
  v.xs = x;
  v.nrhs = 1;
  *yes = (op->M.has_rc && (op->M.rc_tile || march_ok(op->M, v))) ? 1 : 0;
  return MG_OK;
}

// Can mg_op_sweep_residual_dev_FP64 serve this operator with these vectors?  (2-D tile form of the two-stage pass: grid
// operator of z-star classes, relaxPrec bound to the operator and constant per class, x 16-byte aligned.)  *lists: rows the
// pass leaves to mg_op_apply_list_dev_FP64 - list 1 (rows that read the halo: neither t nor r), list 2 (rows next to them: r).
int mg_op_can_sweep_residual(mg_operator* op, const double* x, const double* d, long long* yes, long long* list1, long long* list2) {
  if (!op || !yes) return fail(MG_ERR_INVALID, "null argument");
  const Csr& M = op->M;
  *yes = (M.set && M.has_rc && M.rc_march3 && M.rc_has_d && d && d == M.d_bound && (reinterpret_cast<uintptr_t>(x) & 15) == 0) ? 1 : 0;
  if (list1) *list1 = M.rc_nexc;
  if (list2) *list2 = M.rc_nexc2;
  return MG_OK;
}

// One damped-Jacobi sweep and the residual of its result in ONE pass (csr_rowclass_march3_spmv) over an operator:
//   t = x + d.*(b - M x) on every row that has a class;  r = b - M t [xn = t + d.*r, ||r||^2 partials] on every such row
//   that is not in list 2.  t, r, xn: each optional; d: the relaxPrec bound with mg_op_bind_relax_dev_FP64.
int mg_op_sweep_residual_dev_FP64(mg_operator* op, const double* x, const double* b, const double* d, double* t, double* r,
                                  double* xn, double* partials_dev, long long* nparts, void* stream) {
  if (!op || !op->M.set) return fail(MG_ERR_INVALID, "null or empty operator");
  if (!x || !b || !d || (partials_dev && !nparts)) return fail(MG_ERR_INVALID, "bad argument");
  long long yes = 0;
  MG_TRY(mg_op_can_sweep_residual(op, x, d, &yes, nullptr, nullptr));
  if (!yes) return fail(MG_ERR_UNSUPPORTED, "this operator is not served by the two-stage pass");
  if ((t && (x == t || t == r || t == xn)) || x == r || x == xn || (r && r == xn)) return fail(MG_ERR_INVALID, "x, t, r, xn must be distinct buffers");
  (void)hipSetDevice(op->device);
  const Csr& M = op->M;
  const size_t need = (size_t)12 * 32 * (size_t)M.rm3_nt;
  if (op->m3sink.n < need) MG_TRY(op->m3sink.alloc(need));
  const int o = (r ? 1 : 0) | (xn ? 2 : 0) | (t ? 4 : 0);
  if (!(o == 5 || o == 2 || o == 6 || o == 7) && op->m3scratch.n < (size_t)M.n_rows) MG_TRY(op->m3scratch.alloc((size_t)M.n_rows));
  mgk::March2Args a{};
  a.x = x;
  a.b = b;
  a.t = t;
  a.r = r;
  a.xn = xn;
  a.sumsq = partials_dev;
  a.sink = op->m3sink.p;
  a.d = d;
  MG_TRY(launch_march3_any(reinterpret_cast<hipStream_t>(stream), M, a, false, op->m3scratch.p));
  if (nparts) *nparts = partials_dev ? M.rm3.nblocks : 0;
  return MG_OK;
}

// The rows mg_op_sweep_residual_dev_FP64 leaves out, from the CSR arrays (csr_rows_spmv): list 1 = the rows that read the
// halo, list 2 = the rows next to them.  kernel: MG_K_SMOOTH (y = x + d.*(b - M x)) or MG_K_RESIDUAL (y = b - M x; y2, if
// given, = xs + d.*y with xs = x; partials_dev, if given, receives ||y||^2 partials, *nparts of them).
int mg_op_apply_list_dev_FP64(mg_operator* op, long long list, long long kernel, const double* x, double* y, const double* b,
                              const double* d, double* y2, double* partials_dev, long long* nparts, void* stream) {
  if (!op || !op->M.set) return fail(MG_ERR_INVALID, "null or empty operator");
  if ((list != 1 && list != 2) || !x || !b || (!y && !y2 && !partials_dev) || (partials_dev && !nparts)) return fail(MG_ERR_INVALID, "bad argument");
  if ((kernel == MG_K_SMOOTH || y2) && !d) return fail(MG_ERR_INVALID, "this kernel needs d");
  const Csr& M = op->M;
  const int n = list == 1 ? M.rc_nexc : M.rc_nexc2;
  const int* rows = list == 1 ? M.rc_exc.p : M.rc_exc2.p;
  if (nparts) *nparts = 0;
  if (n <= 0) return MG_OK;
  (void)hipSetDevice(op->device);
  mgk::VecArgs v{};
  v.x = x;
  v.xs = x;
  v.y = y;
  v.b = b;
  v.d = d;
  v.d_full = d;
  v.y2 = y2;
  v.nrhs = 1;
  v.sumsq = partials_dev;
  const int nb = (n + mgk::BLK - 1) / mgk::BLK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (M.wide) return fail(MG_ERR_UNSUPPORTED, "list kernels serve operators with int32 row pointers");
  if (kernel == MG_K_SMOOTH) hipLaunchKernelGGL((mgk::csr_rows_spmv<mgk::SMOOTH>), dim3(nb), dim3(mgk::BLK), 0, s, M.dev(), rows, n, v, 0);
  else if (kernel == MG_K_RESIDUAL) hipLaunchKernelGGL((mgk::csr_rows_spmv<mgk::RESID>), dim3(nb), dim3(mgk::BLK), 0, s, M.dev(), rows, n, v, 0);
  else return fail(MG_ERR_INVALID, "kernel %lld is not a list kernel", kernel);
  HIP_TRY(hipGetLastError());
  if (nparts && partials_dev) *nparts = nb;
  return MG_OK;
}

int mg_op_info(mg_operator* op, long long* n_rows, long long* n_cols, long long* nnz, double* device_bytes) {
  if (!op) return fail(MG_ERR_INVALID, "null operator");
  if (n_rows) *n_rows = op->M.n_rows;
  if (n_cols) *n_cols = op->M.n_cols;
  if (nnz) *nnz = op->M.nnz;
  if (device_bytes) *device_bytes = (double)op->M.bytes();
  return MG_OK;
}

int mg_vec_dscale_dev_FP64(const double* d, const double* b, double* x, long long n, long long nrhs, void* stream) {
  if (!d || !b || !x || n < 1 || nrhs < 1) return fail(MG_ERR_INVALID, "bad vector arguments");
  hipLaunchKernelGGL(mgk::dscale_kernel, dim3(grid_for(n * nrhs / 2 + 1)), dim3(mgk::BLK), 0,
                     reinterpret_cast<hipStream_t>(stream), d, b, x, n, (int)nrhs);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}

int mg_vec_xpdr_dev_FP64(const double* x, const double* d, const double* r, double* xout, long long n,
                         long long nrhs, void* stream) {
  if (!x || !d || !r || !xout || n < 1 || nrhs < 1) return fail(MG_ERR_INVALID, "bad vector arguments");
  hipLaunchKernelGGL(mgk::xpdr_kernel, dim3(grid_for(n * nrhs / 2 + 1)), dim3(mgk::BLK), 0,
                     reinterpret_cast<hipStream_t>(stream), x, d, r, xout, n, (int)nrhs);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}

// out[0] = sum_i x[i]^2 ; workspace: >= 1024 doubles
int mg_vec_sumsq_dev_FP64(const double* x, long long len, double* workspace, double* out, void* stream) {
  if (!x || !workspace || !out || len < 1) return fail(MG_ERR_INVALID, "bad vector arguments");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int nb = (int)std::min<long long>(1024, std::max<long long>(1, (len / 2 + mgk::BLK - 1) / mgk::BLK));
  hipLaunchKernelGGL(mgk::sumsq_partial, dim3(nb), dim3(mgk::BLK), 0, s, x, len, workspace);
  hipLaunchKernelGGL(mgk::sum_final, dim3(1), dim3(mgk::BLK), 0, s, workspace, nb, out);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}

// ---- hybrid Kaczmarz relaxation (deps/src/parRelax.h:7-43) -------------------------------------------------------------
// The four value types of the reference's parRelax.c; a value is kz_bytes[vt] bytes (complex: interleaved re, im).
enum KzType { KZ_FP64 = 0, KZ_CFP64 = 1, KZ_FP32 = 2, KZ_CFP32 = 3 };
static const size_t kz_bytes[4] = {sizeof(double), 2 * sizeof(double), sizeof(float), 2 * sizeof(float)};
static const char* const kz_name[4] = {"FP64", "CFP64", "FP32", "CFP32"};

struct mg_kaczmarz {
  int device = 0;
  KzType vt = KZ_FP64;   // value type of val, invD, x and b, fixed at creation
  long long n = 0, nnz = 0, num_domains = 0, domain_length = 0;
  DevBuf<int> rowptr, col;
  DevBuf<unsigned char> val, invD, x, b;   // sized in bytes: kz_bytes[vt] per value
  DevBuf<unsigned int> arr;
  hipStream_t stream = nullptr;
};

// Every value type: valA and invD hold nnz and n values of kz_bytes[vt] bytes.
static int kaczmarz_create(KzType vt, long long device_id, long long n, const long long* rowptr, const void* valA,
                           const long long* colA, long long numDomains, long long domainLength,
                           const unsigned int* ArrIdxs, const void* invD, mg_kaczmarz** out) {
  const size_t vb = kz_bytes[vt];
  UploadFence upload_fence;
  if (!out) return fail(MG_ERR_INVALID, "out is null");
  *out = nullptr;
  if (n < 1 || !rowptr || !valA || !colA || !ArrIdxs || !invD || numDomains < 1 || domainLength < 1)
    return fail(MG_ERR_INVALID, "null or empty argument");
  if (n >= (1LL << 31) - 1 || numDomains * domainLength >= (1LL << 31)) return fail(MG_ERR_UNSUPPORTED, "dimension exceeds int32 device indices");
  if (rowptr[0] != 1) return fail(MG_ERR_INVALID, "rowptr[1] must be 1 (1-based Julia arrays expected)");
  const long long nnz = rowptr[n] - 1;
  if (nnz < 0 || nnz >= (1LL << 31) - 1) return fail(MG_ERR_UNSUPPORTED, "nnz does not fit int32");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (ndev <= 0) return fail(MG_ERR_HIP, "no HIP device visible: the relaxation has no CPU fallback");
  if (device_id < 0 || device_id >= ndev) return fail(MG_ERR_INVALID, "device_id=%lld but %d devices visible", device_id, ndev);
  std::vector<int> rp((size_t)n + 1), ci((size_t)std::max<long long>(nnz, 1));
  for (long long i = 0; i <= n; ++i) {
    const long long v = rowptr[i] - 1;
    if (v < 0 || v > nnz || (i > 0 && v < rp[(size_t)i - 1])) return fail(MG_ERR_INVALID, "rowptr is not a monotone 1-based pointer array");
    rp[(size_t)i] = (int)v;
  }
  for (long long k = 0; k < nnz; ++k) {
    const long long c = colA[k] - 1;
    if (c < 0 || c >= n) return fail(MG_ERR_INVALID, "column index out of range");
    ci[(size_t)k] = (int)c;
  }
  for (long long t = 0; t < numDomains * domainLength; ++t)
    if ((long long)ArrIdxs[t] > n) return fail(MG_ERR_INVALID, "ArrIdxs entry %u exceeds n=%lld", ArrIdxs[t], n);
  HIP_TRY(hipSetDevice((int)device_id));
  mg_kaczmarz* k = new mg_kaczmarz();
  k->device = (int)device_id;
  k->vt = vt;
  k->n = n;
  k->nnz = nnz;
  k->num_domains = numDomains;
  k->domain_length = domainLength;
  int rc = MG_OK;
  auto up = [&]() -> int {
    MG_TRY(k->rowptr.alloc(rp.size()));
    MG_TRY(k->col.alloc(ci.size()));
    MG_TRY(k->val.alloc(vb * (size_t)std::max<long long>(nnz, 1)));
    MG_TRY(k->invD.alloc(vb * (size_t)n));
    MG_TRY(k->arr.alloc((size_t)(numDomains * domainLength)));
    HIP_TRY(hipMemcpy(k->rowptr.p, rp.data(), rp.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(k->col.p, ci.data(), (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(k->val.p, valA, vb * (size_t)nnz, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(k->invD.p, invD, vb * (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(k->arr.p, ArrIdxs, (size_t)(numDomains * domainLength) * sizeof(unsigned int), hipMemcpyHostToDevice));
    HIP_TRY(hipStreamCreateWithFlags(&k->stream, hipStreamNonBlocking));
    return MG_OK;
  };
  rc = up();
  if (rc != MG_OK) {
    mg_kaczmarz_destroy(k);
    return rc;
  }
  *out = k;
  return MG_OK;
}

int mg_kaczmarz_create_FP64_INT64(long long device_id, long long n, const long long* rowptr, const double* valA,
                                  const long long* colA, long long numDomains, long long domainLength,
                                  const unsigned int* ArrIdxs, const double* invD, mg_kaczmarz** out) {
  return kaczmarz_create(KZ_FP64, device_id, n, rowptr, valA, colA, numDomains, domainLength, ArrIdxs, invD, out);
}

// valA = nzval of the CSC of the reference's AT = A^H (conj of A's CSR values), invD complex: interleaved (re, im) doubles
int mg_kaczmarz_create_CFP64_INT64(long long device_id, long long n, const long long* rowptr, const double* valA,
                                   const long long* colA, long long numDomains, long long domainLength,
                                   const unsigned int* ArrIdxs, const double* invD, mg_kaczmarz** out) {
  return kaczmarz_create(KZ_CFP64, device_id, n, rowptr, valA, colA, numDomains, domainLength, ArrIdxs, invD, out);
}

// The single forms (applyHybridKaczmarz_FP32_INT64 / _CFP32_INT64): valA = AT.nzval and invD in float, interleaved for CFP32
int mg_kaczmarz_create_FP32_INT64(long long device_id, long long n, const long long* rowptr, const float* valA,
                                  const long long* colA, long long numDomains, long long domainLength,
                                  const unsigned int* ArrIdxs, const float* invD, mg_kaczmarz** out) {
  return kaczmarz_create(KZ_FP32, device_id, n, rowptr, valA, colA, numDomains, domainLength, ArrIdxs, invD, out);
}
int mg_kaczmarz_create_CFP32_INT64(long long device_id, long long n, const long long* rowptr, const float* valA,
                                   const long long* colA, long long numDomains, long long domainLength,
                                   const unsigned int* ArrIdxs, const float* invD, mg_kaczmarz** out) {
  return kaczmarz_create(KZ_CFP32, device_id, n, rowptr, valA, colA, numDomains, domainLength, ArrIdxs, invD, out);
}

int mg_kaczmarz_destroy(mg_kaczmarz* k) {
  if (!k) return MG_OK;
  (void)hipSetDevice(k->device);
  if (k->stream) {
    (void)spin_sync(k->stream);
    (void)hipStreamDestroy(k->stream);
  }
  k->rowptr.release();
  k->col.release();
  k->val.release();
  k->invD.release();
  k->arr.release();
  k->x.release();
  k->b.release();
  delete k;
  return MG_OK;
}

// The arguments of an apply and the handle's value type (vt: the entry point's)
static int kaczmarz_args(KzType vt, mg_kaczmarz* k, const void* x, const void* b, long long nrhs, long long numit) {
  if (!k || !x || !b || nrhs < 1 || numit < 0) return fail(MG_ERR_INVALID, "bad argument");
  if (k->vt != vt) {
    if (vt == KZ_CFP64 && k->vt == KZ_FP64)
      return fail(MG_ERR_STATE, "CFP64 Kaczmarz entry point called on an FP64 handle (mg_kaczmarz_create_CFP64_INT64)");
    if (vt == KZ_FP64 && k->vt == KZ_CFP64)
      return fail(MG_ERR_STATE, "FP64 Kaczmarz entry point called on a CFP64 handle (mg_kaczmarz_apply*_CFP64)");
    return fail(MG_ERR_STATE, "%s Kaczmarz entry point called on a %s handle (mg_kaczmarz_apply*_%s)", kz_name[vt], kz_name[k->vt],
                kz_name[k->vt]);
  }
  (void)hipSetDevice(k->device);
  return MG_OK;
}

// one sweep of a single handle: S = float or mgk::f2_t
#define KACZMARZ_LAUNCH_SINGLE(S)                                                                                              \
  hipLaunchKernelGGL(mgk::hybrid_kaczmarz_s<S>, grid, dim3(64), 0, k->stream, k->rowptr.p, k->col.p,                           \
                     reinterpret_cast<const S*>(k->val.p), k->arr.p, (int)k->num_domains, (int)k->domain_length,               \
                     static_cast<S*>(x_dev), static_cast<const S*>(b_dev), (int)nrhs, k->n,                                    \
                     reinterpret_cast<const S*>(k->invD.p), sequential ? 1 : 0)

// numit sweeps on device-resident x (in/out) and b, column-major n x nrhs (complex: interleaved); one launch per sweep
// (the barrier the reference's `omp for` has between sweeps).  sequential != 0: one wavefront walks all sub-domains in
// order (the reference with one thread); otherwise one wavefront per sub-domain.  The single kernels move a value in one
// access: x and b must be aligned to it.
static int kaczmarz_apply_dev(KzType vt, mg_kaczmarz* k, void* x_dev, const void* b_dev, long long nrhs, long long numit,
                              long long sequential) {
  MG_TRY(kaczmarz_args(vt, k, x_dev, b_dev, nrhs, numit));
  if ((vt == KZ_FP32 || vt == KZ_CFP32) &&
      (reinterpret_cast<uintptr_t>(x_dev) % kz_bytes[vt] != 0 || reinterpret_cast<uintptr_t>(b_dev) % kz_bytes[vt] != 0))
    return fail(MG_ERR_INVALID, "x_dev and b_dev must be aligned to %zu bytes (one %s value)", kz_bytes[vt], kz_name[vt]);
  const dim3 grid(sequential ? 1u : (unsigned)k->num_domains);
  for (long long it = 0; it < numit; ++it) {
    if (vt == KZ_CFP64)
      hipLaunchKernelGGL(mgk::hybrid_kaczmarz_c, grid, dim3(64), 0, k->stream, k->rowptr.p, k->col.p,
                         reinterpret_cast<const mgk::d2_t*>(k->val.p), k->arr.p, (int)k->num_domains, (int)k->domain_length,
                         static_cast<double*>(x_dev), static_cast<const double*>(b_dev), (int)nrhs, k->n,
                         reinterpret_cast<const mgk::d2_t*>(k->invD.p), sequential ? 1 : 0);
    else if (vt == KZ_FP64)
      hipLaunchKernelGGL(mgk::hybrid_kaczmarz, grid, dim3(64), 0, k->stream, k->rowptr.p, k->col.p,
                         reinterpret_cast<const double*>(k->val.p), k->arr.p, (int)k->num_domains, (int)k->domain_length,
                         static_cast<double*>(x_dev), static_cast<const double*>(b_dev), (int)nrhs, k->n,
                         reinterpret_cast<const double*>(k->invD.p), sequential ? 1 : 0);
    else if (vt == KZ_CFP32)
      KACZMARZ_LAUNCH_SINGLE(mgk::f2_t);
    else
      KACZMARZ_LAUNCH_SINGLE(float);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(spin_sync(k->stream));
  return MG_OK;
}
#undef KACZMARZ_LAUNCH_SINGLE

// Host buffers, exactly the reference's call (parRelax.jl:61-64 / 71-74): x (in/out) and b are n x nrhs column-major.
static int kaczmarz_apply_host(KzType vt, mg_kaczmarz* k, void* x, const void* b, long long nrhs, long long numit,
                               long long sequential) {
  MG_TRY(kaczmarz_args(vt, k, x, b, nrhs, numit));
  const size_t len = kz_bytes[vt] * (size_t)k->n * (size_t)nrhs;   // bytes
  if (k->x.n != len) {
    MG_TRY(k->x.alloc(len));
    MG_TRY(k->b.alloc(len));
  }
  HIP_TRY(hipMemcpyAsync(k->x.p, x, len, hipMemcpyHostToDevice, k->stream));
  HIP_TRY(hipMemcpyAsync(k->b.p, b, len, hipMemcpyHostToDevice, k->stream));
  MG_TRY(kaczmarz_apply_dev(vt, k, k->x.p, k->b.p, nrhs, numit, sequential));
  HIP_TRY(hipMemcpyAsync(x, k->x.p, len, hipMemcpyDeviceToHost, k->stream));
  HIP_TRY(spin_sync(k->stream));
  return MG_OK;
}

int mg_kaczmarz_apply_dev_FP64(mg_kaczmarz* k, double* x_dev, const double* b_dev, long long nrhs, long long numit,
                               long long sequential) {
  return kaczmarz_apply_dev(KZ_FP64, k, x_dev, b_dev, nrhs, numit, sequential);
}
int mg_kaczmarz_apply_FP64(mg_kaczmarz* k, double* x, const double* b, long long nrhs, long long numit, long long sequential) {
  return kaczmarz_apply_host(KZ_FP64, k, x, b, nrhs, numit, sequential);
}
// The complex sweeps (applyHybridKaczmarz_CFP64_INT64): x and b interleaved complex
int mg_kaczmarz_apply_dev_CFP64(mg_kaczmarz* k, double* x_dev, const double* b_dev, long long nrhs, long long numit,
                                long long sequential) {
  return kaczmarz_apply_dev(KZ_CFP64, k, x_dev, b_dev, nrhs, numit, sequential);
}
int mg_kaczmarz_apply_CFP64(mg_kaczmarz* k, double* x, const double* b, long long nrhs, long long numit, long long sequential) {
  return kaczmarz_apply_host(KZ_CFP64, k, x, b, nrhs, numit, sequential);
}
// The single sweeps (applyHybridKaczmarz_FP32_INT64 / _CFP32_INT64): x and b in float, interleaved for CFP32
int mg_kaczmarz_apply_dev_FP32(mg_kaczmarz* k, float* x_dev, const float* b_dev, long long nrhs, long long numit,
                               long long sequential) {
  return kaczmarz_apply_dev(KZ_FP32, k, x_dev, b_dev, nrhs, numit, sequential);
}
int mg_kaczmarz_apply_FP32(mg_kaczmarz* k, float* x, const float* b, long long nrhs, long long numit, long long sequential) {
  return kaczmarz_apply_host(KZ_FP32, k, x, b, nrhs, numit, sequential);
}
int mg_kaczmarz_apply_dev_CFP32(mg_kaczmarz* k, float* x_dev, const float* b_dev, long long nrhs, long long numit,
                                long long sequential) {
  return kaczmarz_apply_dev(KZ_CFP32, k, x_dev, b_dev, nrhs, numit, sequential);
}
int mg_kaczmarz_apply_CFP32(mg_kaczmarz* k, float* x, const float* b, long long nrhs, long long numit, long long sequential) {
  return kaczmarz_apply_host(KZ_CFP32, k, x, b, nrhs, numit, sequential);
}

// Run the hierarchy's kernels on the caller's stream (e.g. torch's current stream) instead of its own.
int mg_set_stream(mg_hierarchy* h, void* stream) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  graphs_clear(h);
  (void)hipSetDevice(h->device);
  (void)spin_sync(h->lane0.stream);
  if (h->lane0.owns_stream && h->lane0.stream) (void)hipStreamDestroy(h->lane0.stream);
  h->lane0.stream = reinterpret_cast<hipStream_t>(stream);
  h->lane0.owns_stream = false;
  return MG_OK;
}

// Enqueue one cycle and return without waiting (x_is_zero must be 0 or 1).
int mg_cycle_async_dev_FP64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs,
                            long long x_is_zero) {
  MG_REAL_ONLY(h);
  MG_TRY(check_ready(h, n, nrhs));
  if (!b || !x) return fail(MG_ERR_INVALID, "null vector");
  if (x_is_zero != 0 && x_is_zero != 1) return fail(MG_ERR_INVALID, "x_is_zero must be 0 or 1 for the asynchronous cycle");
  (void)hipSetDevice(h->device);
  return cycle_dev(h, b, x, x_is_zero == 1);
}

// The K-cycle's step INTO this hierarchy's first level (MGcycle.jl:72-76): x = 2 steps of FGMRES on A_1 x = b from x = 0,
// preconditioned by the K-cycle of level 1.  For a hierarchy that is the replicated tail of a sharded one (mg_dist_*): the
// level above it is sharded and its K-branch lands here.  A one-level hierarchy just solves.  Asynchronous like
// mg_cycle_async_dev_FP64 as far as the stream goes (the FGMRES dots are host-visible, as everywhere in a K-cycle).
int mg_kcycle_step_async_dev_FP64(mg_hierarchy* h, const double* b, double* x, long long n) {
  MG_CF64_UNSUPPORTED(h);
  MG_TRY(check_ready(h, n, 1));
  if (!b || !x) return fail(MG_ERR_INVALID, "null vector");
  (void)hipSetDevice(h->device);
  if (h->nlevels < 2) return cycle_dev(h, b, x, true);
  if (h->kstepZ.n != (size_t)(2 * n)) {
    MG_TRY(h->kstepZ.alloc((size_t)(2 * n)));
    MG_TRY(h->kstepAZ.alloc((size_t)(2 * n)));
    MG_TRY(h->kstepX.alloc((size_t)n));
  }
  auto kprec = [&](const double* v, double* z) {
    double* res = nullptr;
    MG_TRY(cycle_level(h, 0, v, h->kstepX.p, h->play->lev[0].x1.p, true, 'K', &res));
    HIP_TRY(hipMemcpyAsync(z, res, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, h->play->stream));
    return (int)MG_OK;
  };
  return fgmres_relax(h, 0, b, x, 2, kprec, 1e-5, h->kstepZ.p, h->kstepAZ.p, true);
}

// =================================================================================================================
// Ghost-layer form of the sharded cycle (mg_ghost_*; mg_ghost.inc): the rank's hierarchy is an ordinary mg_hierarchy on
// extended boxes; these calls attach the geometry, the exchange plans and the transport to it.  After mg_ghost_finalize
// mg_cycle_dev_FP64 / mg_solve_dev_FP64 (one right-hand side) run the sharded cycle: b and x are n_ext long (the extended
// fine box), b's owned rows must be valid, x's owned rows are valid on return; norms are over all ranks' owned rows.
// =================================================================================================================
int mg_ghost_attach(mg_hierarchy* h, long long rank, long long world, long long nlevels_sharded, const char* unique_id128) {
  MG_CF64_UNSUPPORTED(h);
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  if (world < 1 || rank < 0 || rank >= world || nlevels_sharded < 1 || nlevels_sharded >= h->nlevels)
    return fail(MG_ERR_INVALID, "bad rank/world/levels (%lld/%lld, %lld sharded of %lld)", rank, world, nlevels_sharded, h->nlevels);
  if (h->coarse_gmres)
    return fail(MG_ERR_UNSUPPORTED, "the ghost-layer form needs a direct coarsest solve (coarseSolveType GMRES: mg_dist_*)");
  if (h->coarse_dd) return fail(MG_ERR_UNSUPPORTED, "a Schwarz sweep as coarsest solve (mg_set_coarse_dd) is not served on sharded hierarchies");
  (void)hipSetDevice(h->device);
  graphs_clear(h);
  if (h->ghost) { gh_release(h->ghost); h->ghost = nullptr; }
  mg_ghost* g = new mg_ghost();
  g->T.rank = (int)rank;
  g->T.world = (int)world;
  g->a = (int)nlevels_sharded;
  g->lev.resize((size_t)nlevels_sharded);
  auto bail = [&](int rc) { gh_release(g); return rc; };
  if (hipStreamCreateWithFlags(&g->side, hipStreamNonBlocking) != hipSuccess || hipHostMalloc(reinterpret_cast<void**>(&g->h_norm), sizeof(double)) != hipSuccess)
    return bail(fail(MG_ERR_HIP, "stream / scratch creation failed"));
  if (unique_id128) {
    const int rc = g->T.init_rccl(unique_id128);
    if (rc != MG_OK) return bail(rc);
  }
  h->ghost = g;
  return MG_OK;
}

// A second RCCL communicator (another id of mg_dist_unique_id, broadcast like the first) for the ghost-layer send / recv on the
// side stream: RCCL serialises the operations of ONE communicator in issue order, whatever their streams; with its own
// communicator the fine level's exchange runs beside the coarse cycle and its all-reduces instead of in front of them.
int mg_ghost_set_side_comm(mg_hierarchy* h, const char* unique_id128) {
  MG_CF64_UNSUPPORTED(h);
  if (!h || !h->ghost || !unique_id128) return fail(MG_ERR_INVALID, "null argument or mg_ghost_attach was not called");
  (void)hipSetDevice(h->device);
  return h->ghost->T.init_side(unique_id128);
}

int mg_ghost_set_exchange_plugin(mg_hierarchy* h, mg_exchange_fn fn, void* user) {
  MG_CF64_UNSUPPORTED(h);
  if (!h || !h->ghost) return fail(MG_ERR_INVALID, "null argument or mg_ghost_attach was not called");
  return h->ghost->T.set_plugin(fn, user);
}

// Sharded level `level` (1-based): extended box ext[3] (nodes per dimension, x fastest; 1 for unused dimensions), owned box
// [own_lo, own_hi) inside it, gmin = the smallest ghost width over the cut sides OF ANY RANK (the schedule of exchanges must
// be the same on every rank); send_idx: extended-box ids (0-based) of owned nodes grouped by destination rank
// (send_splits[world]); recv_idx: extended-box ids of this rank's ghost nodes grouped by owner (recv_splits[world]), each
// peer's part in ascending global id on both sides.
int mg_ghost_set_level_INT64(mg_hierarchy* h, long long level, const long long* ext, const long long* own_lo, const long long* own_hi,
                             long long gmin, long long n_send, const long long* send_idx, const long long* send_splits,
                             long long n_recv, const long long* recv_idx, const long long* recv_splits) {
  MG_CF64_UNSUPPORTED(h);
  UploadFence upload_fence;
  if (!h || !h->ghost) return fail(MG_ERR_INVALID, "mg_ghost_attach was not called");
  mg_ghost* g = h->ghost;
  if (level < 1 || level > g->a) return fail(MG_ERR_INVALID, "bad level %lld", level);
  if (!ext || !own_lo || !own_hi || !send_splits || !recv_splits || (n_send > 0 && !send_idx) || (n_recv > 0 && !recv_idx) || n_send < 0 || n_recv < 0 || gmin < 1)
    return fail(MG_ERR_INVALID, "bad ghost-level arrays");
  (void)hipSetDevice(h->device);
  GhostLevel& L = g->lev[(size_t)level - 1];
  long long n = 1;
  for (int k = 0; k < 3; ++k) {
    if (ext[k] < 1 || own_lo[k] < 0 || own_hi[k] <= own_lo[k] || own_hi[k] > ext[k]) return fail(MG_ERR_INVALID, "ghost level %lld: bad boxes", level);
    L.ext[k] = (int)ext[k]; L.lo[k] = (int)own_lo[k]; L.hi[k] = (int)own_hi[k];
    n *= ext[k];
  }
  if (n != h->lev[(size_t)level - 1].A.n_rows && h->lev[(size_t)level - 1].A.set)
    return fail(MG_ERR_INVALID, "ghost level %lld: the extended box has %lld nodes, As[%lld] %lld rows", level, n, level, h->lev[(size_t)level - 1].A.n_rows);
  L.n = n;
  L.gmin = (int)std::min<long long>(gmin, GH_FULL);
  L.n_send = n_send;
  L.n_recv = n_recv;
  L.send_splits.assign(send_splits, send_splits + g->T.world);
  L.recv_splits.assign(recv_splits, recv_splits + g->T.world);
  long long ss = 0, rs = 0;
  for (int q = 0; q < g->T.world; ++q) { ss += L.send_splits[(size_t)q]; rs += L.recv_splits[(size_t)q]; }
  if (ss != n_send || rs != n_recv) return fail(MG_ERR_INVALID, "ghost plan: splits do not add up (send %lld/%lld, recv %lld/%lld)", ss, n_send, rs, n_recv);
  auto in_own = [&](long long id) {
    const long long x = id % L.ext[0], y = (id / L.ext[0]) % L.ext[1], z = id / ((long long)L.ext[0] * L.ext[1]);
    return x >= L.lo[0] && x < L.hi[0] && y >= L.lo[1] && y < L.hi[1] && z >= L.lo[2] && z < L.hi[2];
  };
  std::vector<int> si((size_t)std::max<long long>(n_send, 1), 0), ri((size_t)std::max<long long>(n_recv, 1), 0);
  for (long long i = 0; i < n_send; ++i) {
    if (send_idx[i] < 0 || send_idx[i] >= n || !in_own(send_idx[i])) return fail(MG_ERR_INVALID, "ghost plan: a send index is not an owned node");
    si[(size_t)i] = (int)send_idx[i];
  }
  for (long long i = 0; i < n_recv; ++i) {
    if (recv_idx[i] < 0 || recv_idx[i] >= n || in_own(recv_idx[i])) return fail(MG_ERR_INVALID, "ghost plan: a receive index is not a ghost node");
    ri[(size_t)i] = (int)recv_idx[i];
  }
  MG_TRY(L.send_idx.alloc(si.size()));
  MG_TRY(L.recv_idx.alloc(ri.size()));
  MG_TRY(L.send_buf.alloc(si.size()));
  MG_TRY(L.recv_buf.alloc(ri.size()));
  MG_TRY(L.send_buf2.alloc(si.size()));
  MG_TRY(L.recv_buf2.alloc(ri.size()));
  HIP_TRY(hipMemcpy(L.send_idx.p, si.data(), si.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(L.recv_idx.p, ri.data(), ri.size() * sizeof(int), hipMemcpyHostToDevice));
  if (!L.ev_packed) HIP_TRY(hipEventCreateWithFlags(&L.ev_packed, hipEventDisableTiming));
  if (!L.ev_landed) HIP_TRY(hipEventCreateWithFlags(&L.ev_landed, hipEventDisableTiming));
  L.set = true;
  g->finalized = false;
  return MG_OK;
}

int mg_ghost_finalize(mg_hierarchy* h) {
  MG_CF64_UNSUPPORTED(h);
  UploadFence upload_fence;
  if (!h || !h->ghost) return fail(MG_ERR_INVALID, "mg_ghost_attach was not called");
  if (!h->finalized) return fail(MG_ERR_STATE, "hierarchy not finalized: call mg_finalize first");
  mg_ghost* g = h->ghost;
  (void)hipSetDevice(h->device);
  graphs_clear(h);
  MG_TRY(g->T.ready());
  for (int l = 0; l < g->a; ++l) {
    GhostLevel& L = g->lev[(size_t)l];
    if (!L.set) return fail(MG_ERR_STATE, "ghost level %d was not set", l + 1);
    if (L.n != h->lev[(size_t)l].n) return fail(MG_ERR_INVALID, "ghost level %d: the extended box has %lld nodes, the level %lld rows", l + 1, L.n, h->lev[(size_t)l].n);
    L.active = g->T.world > 1;     // (every box of a partition into more than one has a neighbour)
    L.depth.clear();
    L.pending = nullptr;
  }
  MG_TRY(g->b0.alloc((size_t)g->lev[0].n));
  HIP_TRY(hipMemset(g->b0.p, 0, g->b0.bytes()));
  // ---- what EVERY rank's kernels can do (see mg_ghost): one all-reduce of 0/1 flags, a capability is kept where the sum is `world` ----
  {
    const int a = g->a;
    std::vector<double> flags((size_t)(1 + 3 * a), 0.0);
    {
      Level& L0 = h->lev[0];
      flags[0] = (h->nrhs >= 1 && march4_ok_static(h, 0)) ? 1.0 : 0.0;
      for (int l = 0; l < a; ++l) {
        Level& L = h->lev[(size_t)l];
        const bool m2 = march2_ok_static(h, l);
        flags[(size_t)(1 + 3 * l)] = m2 ? 1.0 : 0.0;
        flags[(size_t)(2 + 3 * l)] = (m2 && zero_form_static(L.A)) ? 1.0 : 0.0;
        flags[(size_t)(3 + 3 * l)] = restrict_can_scale_static(h, L.R) ? 1.0 : 0.0;
      }
      (void)L0;
    }
    // the flags travel like every other host-visible sum: staged through pinned memory and all-reduced on ONE stream.  Not a
    // collective of the schedule: mg_ghost_allreduce_count leaves it out.
    const size_t cnt = flags.size();
    const long long counted = g->T.n_allreduce;
    DevBuf<double> tmp;
    MG_TRY(tmp.alloc(cnt));
    MG_TRY(g->T.stage(cnt, h->play->stream));
    double* sums = g->T.h_stage;
    std::copy(flags.begin(), flags.end(), sums);
    HIP_TRY(hipMemcpyAsync(tmp.p, sums, cnt * sizeof(double), hipMemcpyHostToDevice, h->play->stream));
    MG_TRY(g->T.allreduce_now(tmp.p, cnt, sums, h->play->stream));
    tmp.release();
    g->T.n_allreduce = counted;
    const double ranks = g->T.sums_global() ? (double)g->T.world : 1.0;   // (how many ranks' flags a sum holds)
    auto all = [&](size_t i) { return sums[i] > ranks - 0.5; };
    g->agree4 = all(0);
    g->agree2.assign((size_t)a, 1);
    g->agree_zero.assign((size_t)a, 1);
    g->agree_scale.assign((size_t)a, 1);
    for (int l = 0; l < a; ++l) {
      g->agree2[(size_t)l] = all((size_t)(1 + 3 * l)) ? 1 : 0;
      g->agree_zero[(size_t)l] = all((size_t)(2 + 3 * l)) ? 1 : 0;
      g->agree_scale[(size_t)l] = all((size_t)(3 + 3 * l)) ? 1 : 0;
    }
  }
  g->finalized = true;               // (columns_ok reads the agreed flags through the finalized handle)
  if (h->nrhs != 1 && !columns_ok(h)) {    // (every rank sees the same agreed flags: all of them fail here, or none)
    g->finalized = false;
    return fail(MG_ERR_UNSUPPORTED, "ghost-layer form: a block of right-hand sides is solved column by column, which needs: %s", columns_why_not(h));
  }
  return MG_OK;
}

// Timing aid (bench.py --ghost-dry R/N): this process is rank R of a world of N ALONE on its GPU - every exchange runs its pack and
// unpack kernels, nothing travels, sums stay local.  The numbers such a handle computes mean nothing; its step time is what one
// GPU of the N spends on compute, redundant ghost rows included (the ceiling of the strong scaling with free communication).
int mg_ghost_set_dry(mg_hierarchy* h, long long on) {
  MG_CF64_UNSUPPORTED(h);
  if (!h || !h->ghost) return fail(MG_ERR_INVALID, "mg_ghost_attach was not called");
  return h->ghost->T.set_dry(on != 0);
}
// exchanges started and doubles sent by this rank since mg_ghost_attach (what the schedule really communicates)
int mg_ghost_stats(mg_hierarchy* h, long long* exchanges, long long* doubles_sent) {
  MG_CF64_UNSUPPORTED(h);
  if (!h || !h->ghost) return fail(MG_ERR_INVALID, "mg_ghost_attach was not called");
  if (exchanges) *exchanges = h->ghost->T.n_exchanges;
  if (doubles_sent) *doubles_sent = h->ghost->T.n_sent;
  return MG_OK;
}
int mg_ghost_allreduce_count(mg_hierarchy* h, long long* count) {
  MG_CF64_UNSUPPORTED(h);
  if (!h || !h->ghost || !count) return fail(MG_ERR_INVALID, "null argument or mg_ghost_attach was not called");
  *count = h->ghost->T.n_allreduce;
  return MG_OK;
}
// Ranks of this handle's communicator AS RCCL REPORTS THEM (ncclCommCount); 0 with the plug-in transport / a world of one without RCCL.
int mg_ghost_comm_count(mg_hierarchy* h, long long* count) {
  MG_CF64_UNSUPPORTED(h);
  if (!h || !h->ghost || !count) return fail(MG_ERR_INVALID, "null argument or mg_ghost_attach was not called");
  return h->ghost->T.comm_count(count);
}

}  // extern "C"
