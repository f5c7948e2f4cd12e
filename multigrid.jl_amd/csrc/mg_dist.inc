// mg_dist.inc - part of libmgvcycle.so's single translation unit (included by mgvcycle.hip in this order; not compiled on its own).
// Native multi-GPU sequencer (mg_dist_*), the halo form: sharded level schedule, halo exchange on a side stream, replicated tail.
extern "C" {
// =================================================================================================================
// Native multi-GPU sequencer (one process per GPU): the level schedule of the sharded cycle in C++, halo exchange by
// RCCL send/recv on a side stream overlapped with the interior rows, scalar all-reduce for the norm, replicated tail.
// Partition: the reference's DomainDecomposition box rule (DDIndices.jl:41-47, DDService.jl:27-48); worker map analogue:
// DDParallel.jl:105,133-139.  The host (multigrid.jl_amd/distributed.py, or the Julia glue) cuts the hierarchy into
// local operators [owned | halo] and send lists; this code owns the vectors and the hot loop.
// =================================================================================================================
namespace {
struct DistPlan {
  bool set = false, active = false;
  long long n_own_src = 0, n_halo = 0, n_send = 0;
  DevBuf<int> send_idx;
  DevBuf<double> send_buf;
  std::vector<long long> send_splits, recv_splits;   // per peer
};
struct DistLevel {
  long long n_own = 0, n_int = 0;
  mg_operator *A_int = nullptr, *A_bnd = nullptr, *P = nullptr, *R = nullptr;   // borrowed handles
  const double* d = nullptr;                                                    // borrowed device vector (n_own)
  long long npre = 1, npost = 1;
  long long npre_raw = 1, npost_raw = 1;   // relaxPre/relaxPost(level) as given: the inner dimension of a Jac-GMRES relaxation
  DevBuf<double> relZ, relAZ;              // FGMRESmem (FGMRES.jl:3-8) of the Jac-GMRES smoother: Z (with halo tail each), A*Z
  DevBuf<double> kZ, kAZ;                  // memKcycle: the 2-step FGMRES of a K-cycle INTO this level
  bool box = false;   // A_int is a box operator (mg_op_create_box_FP64_INT64): phase 1 overlaps the exchange, phase 2 follows it
  DistPlan planA, planR, planP;
  long long cap_x = 0, cap_r = 0;
  DevBuf<double> x0, x1, r, b;
  DevBuf<double> x2;   // fine level, solve loop: third rotating buffer of the fused last sweep + residual (allocated on first use)
};
// Work space of the sharded Krylov drivers (mg_dist_krylov.inc), allocated at their first call and kept on the handle
struct DistKrylov {
  DevBuf<double> vec;      // the drivers' vectors, carved out of one allocation
  DevBuf<double> part;     // partial sums of the fused passes: MAXS scalars x MAXB workgroups
  DevBuf<double> scal;     // MAXS scalars, all-reduced in place
  double* h_scal = nullptr;   // pinned: the MAXS scalars summed over the ranks, as the host reads them
  void release() {
    vec.release();
    part.release();
    scal.release();
    if (h_scal) (void)hipHostFree(h_scal);
    h_scal = nullptr;
  }
};
}  // namespace

// rows of a row-major block [n][k]: dst row i = src row idx[i]
__global__ __launch_bounds__(256) void dist_pack(const double* __restrict__ src, const int* __restrict__ idx,
                                                 double* __restrict__ dst, long long n, int k) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < n * k) {
    const long long i = e / k;
    dst[e] = src[(long long)idx[i] * k + (e - i * k)];
  }
}
__global__ __launch_bounds__(256) void dist_gather64(const double* __restrict__ src, const long long* __restrict__ idx,
                                                     double* __restrict__ dst, long long n, int k) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < n * k) {
    const long long i = e / k;
    dst[e] = src[idx[i] * k + (e - i * k)];
  }
}

struct mg_dist {
  int device = 0;
  Transport T;
  hipStream_t stream = nullptr, side = nullptr;
  hipEvent_t ev_packed = nullptr, ev_landed = nullptr;
  std::vector<DistLevel> lev;
  char cycle = 'V';
  int relax_type = 0;                   // 0: pointwise (Jac / SPAI), 1: Jac-GMRES (MGcycle.jl:48-50,96-98)
  bool finalized = false;
  long long nrhs = 1;                   // right-hand sides per call (blocks are row-major [n][nrhs], as in mg_hierarchy)
  bool no_pair = false;                 // MG_DIST_NO_PAIR=1: never fuse a sweep with the residual that follows it (A/B, tests)
  // replicated tail
  mg_hierarchy* tail = nullptr;
  // what the tail's handle looked like before this sequencer borrowed it (restored by mg_dist_release_tail / destroy)
  hipStream_t tail_prev_stream = nullptr;
  bool tail_prev_owns = false, tail_prev_no_graph = false, tail_borrowed = false;
  long long n_tail = 0, own_tail = 0, max_tail = 0, nl_total = 0;
  DevBuf<double> bc_pad, bc_all, b_tail, x_tail;
  DevBuf<long long> gather_index;
  // reductions
  DevBuf<double> partial, partial2, scalar;
  double* h_scalar = nullptr;
  DistKrylov kry;
};

namespace {
// Start filling the halo tail buf[n_own_src : n_own_src + n_halo] (values the peers need are packed first).
// RCCL: pack on the compute stream, send/recv on the side stream; the compute stream goes on.  Plug-in: done on return.
int dist_exchange_start(mg_dist* h, DistPlan& p, double* buf) {
  if (!p.set || !p.active) return MG_OK;
  const long long k = h->nrhs;
  if (p.n_send > 0)
    hipLaunchKernelGGL(dist_pack, dim3((unsigned)((p.n_send * k + 255) / 256)), dim3(256), 0, h->stream, buf, p.send_idx.p, p.send_buf.p, p.n_send, (int)k);
  HIP_TRY(hipGetLastError());
  const bool hop = h->T.on_stream();
  if (hop) {
    HIP_TRY(hipEventRecord(h->ev_packed, h->stream));
    HIP_TRY(hipStreamWaitEvent(h->side, h->ev_packed, 0));
  }
  const Transport::Pair pair = {p.send_buf.p, buf + p.n_own_src * k};   // (received straight into the halo tail)
  MG_TRY(h->T.exchange(&pair, 1, p.send_splits, p.recv_splits, k, hop ? h->side : h->stream));
  if (hop) HIP_TRY(hipEventRecord(h->ev_landed, h->side));
  return MG_OK;
}
// Make the compute stream wait for the halo started by dist_exchange_start.
int dist_exchange_finish(mg_dist* h, DistPlan& p) {
  if (!p.set || !p.active) return MG_OK;
  if (h->T.on_stream()) HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_landed, 0));
  return MG_OK;
}

int dist_apply(mg_dist* h, mg_operator* op, long long kernel, double alpha, const double* x, double beta, double* y,
               const double* b, const double* d, long long row_offset) {
  if (!op) return MG_OK;
  return mg_op_apply_rows_dev_FP64(op, kernel, alpha, x, beta, y, b, d, h->nrhs, row_offset, h->stream);
}
// out = b - A x / out = x + d.*(b - A x) on this rank's rows, the halo exchange overlapped with the interior rows
int dist_apply_A(mg_dist* h, DistLevel& L, long long kernel, double* x, double* out, const double* b) {
  MG_TRY(dist_exchange_start(h, L.planA, x));
  if (L.box) {   // rows of the owned box that do not read the halo (staged kernels), then - halo landed - the rest
    MG_TRY(mg_op_apply_phase_dev_FP64(L.A_int, kernel, 1.0, x, 0.0, out, b, L.d, h->nrhs, 0, 1, h->stream));
    MG_TRY(dist_exchange_finish(h, L.planA));
    MG_TRY(mg_op_apply_phase_dev_FP64(L.A_int, kernel, 1.0, x, 0.0, out, b, L.d, h->nrhs, 0, 2, h->stream));
    return MG_OK;
  }
  MG_TRY(dist_apply(h, L.A_int, kernel, 1.0, x, 0.0, out, b, L.d, 0));
  MG_TRY(dist_exchange_finish(h, L.planA));
  MG_TRY(dist_apply(h, L.A_bnd, kernel, 1.0, x, 0.0, out, b, L.d, L.n_int));
  return MG_OK;
}
// global Frobenius norm of a sharded vector: local sum of squares + one scalar all-reduce (SolveFuncs.jl:15,20,30)
int dist_reduce_scalar(mg_dist* h, double* out);
int dist_norm(mg_dist* h, const double* v, long long n, double* out) {
  MG_TRY(mg_vec_sumsq_dev_FP64(v, n, h->partial.p, h->scalar.p, h->stream));
  return dist_reduce_scalar(h, out);
}

// all-reduce h->scalar (a local sum of squares) and return its square root on the host
int dist_reduce_scalar(mg_dist* h, double* out) {
  MG_TRY(h->T.allreduce_now(h->scalar.p, 1, h->h_scalar, h->stream));
  *out = std::sqrt(*h->h_scalar);
  return MG_OK;
}

// Can the sweep + residual pair of this level run as one two-stage pass (box-form level whose A is on the 2-D tile form)?
bool dist_pair_ok(mg_dist* h, DistLevel& L, const double* x) {
  if (!L.box || h->relax_type != 0 || h->no_pair || !L.A_int || h->nrhs != 1) return false;
  long long yes = 0;
  if (mg_op_can_sweep_residual(L.A_int, x, L.d, &yes, nullptr, nullptr) != MG_OK) return false;
  return yes != 0;
}
// One sweep and the residual of its result on a sharded box-form level (MGcycle.jl:54-60; SolveFuncs.jl:26-30 with the last
// post-smoothing sweep): t = x + d.*(b - A x), r = b - A t [, xn = t + d.*r, ||r|| over all ranks].  Two exchanges as for
// the two launches it replaces, one pass over the level instead of two:
//   exchange(x) || two-stage pass: t everywhere but on the rows that read the halo, r two layers in
//   -> t on those rows -> exchange(t) || r of the layer behind them -> r on them.
// t: a buffer with a halo tail (cap_x).  r / xn: each optional.
int dist_sweep_residual(mg_dist* h, DistLevel& L, double* x, double* t, double* r, double* xn, const double* b, double* norm) {
  long long n0 = 0, n1 = 0, n2 = 0;
  double* part = norm ? h->partial.p : nullptr;
  if (norm) {
    const Csr& M = L.A_int->M;
    const size_t need = (size_t)M.rm3.nblocks + (size_t)(M.rc_nexc + M.rc_nexc2) / mgk::BLK + 4;
    if (need > h->partial.n) return fail(MG_ERR_STATE, "partial-sum buffer too small (%zu > %zu)", need, h->partial.n);
  }
  MG_TRY(dist_exchange_start(h, L.planA, x));
  MG_TRY(mg_op_sweep_residual_dev_FP64(L.A_int, x, b, L.d, t, r, xn, part, &n0, h->stream));
  MG_TRY(dist_exchange_finish(h, L.planA));
  MG_TRY(mg_op_apply_list_dev_FP64(L.A_int, 1, MG_K_SMOOTH, x, t, b, L.d, nullptr, nullptr, nullptr, h->stream));
  MG_TRY(dist_exchange_start(h, L.planA, t));
  MG_TRY(mg_op_apply_list_dev_FP64(L.A_int, 2, MG_K_RESIDUAL, t, r, b, L.d, xn, part ? part + n0 : nullptr, &n1, h->stream));
  MG_TRY(dist_exchange_finish(h, L.planA));
  MG_TRY(mg_op_apply_list_dev_FP64(L.A_int, 1, MG_K_RESIDUAL, t, r, b, L.d, xn, part ? part + n0 + n1 : nullptr, &n2, h->stream));
  if (norm) {
    const long long nb1 = n0 + n1 + n2;
    const int nb2 = (int)std::min<long long>(256, (nb1 + mgk::BLK - 1) / mgk::BLK);
    hipLaunchKernelGGL(mgk::sum_partial, dim3(nb2), dim3(mgk::BLK), 0, h->stream, h->partial.p, nb1, h->partial2.p);
    hipLaunchKernelGGL(mgk::sum_final, dim3(1), dim3(mgk::BLK), 0, h->stream, h->partial2.p, nb2, h->scalar.p);
    HIP_TRY(hipGetLastError());
    MG_TRY(dist_reduce_scalar(h, norm));
  }
  return MG_OK;
}

// SolveFuncs.jl:26-30 on the sharded fine level: r = b - A x and ||r|| in ONE pass over the level (per-workgroup partial
// sums, one scalar all-reduce).  Box-form levels also get alt = x + d.*r, the next cycle's first damped-Jacobi update,
// from the same pass (*x1_ready), and then do not store r at all - as solve_dev does on one GPU.
int dist_residual_norm(mg_dist* h, DistLevel& L, double* x, const double* b, double* alt, double* norm, bool* x1_ready) {
  *x1_ready = false;
  long long can = 0;
  if (L.box && alt && h->nrhs == 1) MG_TRY(mg_op_can_fuse_next(L.A_int, x, &can));
  if (!L.box || h->nrhs != 1) {     // (blocks: the Frobenius norm over the whole n x nrhs block, SolveFuncs.jl:30)
    MG_TRY(dist_apply_A(h, L, MG_K_RESIDUAL, x, L.r.p, b));
    return dist_norm(h, L.r.p, L.n_own * h->nrhs, norm);
  }
  long long n1 = 0, n2 = 0;
  {   // capacity before anything is written: every launch form of this operator writes at most this many partials
    const Csr& M = L.A_int->M;
    const size_t need = (size_t)std::max(M.blocks1(), M.nblocks) + (size_t)(M.rc_nexc + mgk::BLK - 1) / mgk::BLK + 1;
    if (need > h->partial.n) return fail(MG_ERR_STATE, "partial-sum buffer too small (%zu > %zu)", need, h->partial.n);
  }
  MG_TRY(dist_exchange_start(h, L.planA, x));
  MG_TRY(mg_op_residual_fused_dev_FP64(L.A_int, x, b, L.d, can ? nullptr : L.r.p, can ? alt : nullptr, h->partial.p, 1, &n1, h->stream));
  MG_TRY(dist_exchange_finish(h, L.planA));
  MG_TRY(mg_op_residual_fused_dev_FP64(L.A_int, x, b, L.d, can ? nullptr : L.r.p, can ? alt : nullptr, h->partial.p + n1, 2, &n2, h->stream));
  const long long nb1 = n1 + n2;
  if (nb1 <= 0) return fail(MG_ERR_STATE, "the fused residual wrote no partial sums");
  const int nb2 = (int)std::min<long long>(256, (nb1 + mgk::BLK - 1) / mgk::BLK);
  hipLaunchKernelGGL(mgk::sum_partial, dim3(nb2), dim3(mgk::BLK), 0, h->stream, h->partial.p, nb1, h->partial2.p);
  hipLaunchKernelGGL(mgk::sum_final, dim3(1), dim3(mgk::BLK), 0, h->stream, h->partial2.p, nb2, h->scalar.p);
  HIP_TRY(hipGetLastError());
  MG_TRY(dist_reduce_scalar(h, norm));
  *x1_ready = can != 0;
  return MG_OK;
}

// dot(x, y) over all ranks (local partial sums + one scalar all-reduce); the same bits on every rank
int dist_dot(mg_dist* h, const double* x, const double* y, long long n, double* out) {
  const int nb = (int)std::max<long long>(1, std::min<long long>((long long)h->partial.n, (n / 2 + mgk::BLK - 1) / mgk::BLK));
  hipLaunchKernelGGL(mgk::dot_partial, dim3(nb), dim3(mgk::BLK), 0, h->stream, x, y, n, h->partial.p);
  hipLaunchKernelGGL(mgk::sum_final, dim3(1), dim3(mgk::BLK), 0, h->stream, h->partial.p, nb, h->scalar.p);
  HIP_TRY(hipGetLastError());
  double nrm = 0.0;
  MG_TRY(dist_reduce_scalar(h, &nrm));   // sqrt of the all-reduced sum ...
  *out = *h->h_scalar;                   // ... whose raw value stays in the pinned scalar
  return MG_OK;
}
int dist_axpby(mg_dist* h, double a, const double* x, double b, double* y, long long n) {
  hipLaunchKernelGGL(mgk::axpby_kernel, dim3(grid_for(n)), dim3(mgk::BLK), 0, h->stream, a, x, b, y, n);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
int dist_fill(mg_dist* h, double* x, long long n, double val) {
  hipLaunchKernelGGL(mgk::fill_kernel, dim3(grid_for(n)), dim3(mgk::BLK), 0, h->stream, x, n, val);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
// FGMRES_relaxation (FGMRES.jl:48-126) on a sharded level - the mirror of fgmres_relax, sharing its least squares (RelaxLsq): x0 += Z*t where t minimises
// ||r0 - A Z t|| over the `inner` directions z_1 = M r0, z_j = M (A z_{j-1}).  Products with A exchange the halo of z (the
// vectors of Z are cap_x long: owned rows + halo tail), dots are all-reduced, so the small pseudo-inverse and the
// data-dependent exit (l.114-117) come out identical on every rank.
extern "C++" {
template <class Prec>
int dist_fgmres_relax(mg_dist* h, DistLevel& L, const double* r0, double* x0, long long inner, Prec prec, double TOL,
                      DevBuf<double>& Zbuf, DevBuf<double>& AZbuf, bool x0_is_zero) {
  const long long n = L.n_own;
  if (inner <= 0) {
    if (x0_is_zero) MG_TRY(dist_fill(h, x0, n, 0.0));
    return MG_OK;  // w = Z*t with no columns: x0 unchanged (FGMRES.jl:119-121)
  }
  const int k = (int)inner;
  if (Zbuf.n < (size_t)k * (size_t)L.cap_x) {
    MG_TRY(Zbuf.alloc((size_t)k * (size_t)L.cap_x));
    HIP_TRY(hipMemsetAsync(Zbuf.p, 0, Zbuf.bytes(), h->stream));
  }
  if (AZbuf.n < (size_t)k * (size_t)n) MG_TRY(AZbuf.alloc((size_t)k * (size_t)n));
  double rnorm0 = 0.0;
  MG_TRY(dist_norm(h, r0, n, &rnorm0));
  RelaxLsq Q(k);
  int used = 0;
  for (int j = 0; j < k; ++j) {
    double* z = Zbuf.p + (size_t)j * (size_t)L.cap_x;
    double* w = AZbuf.p + (size_t)j * (size_t)n;
    MG_TRY(prec(j == 0 ? r0 : AZbuf.p + (size_t)(j - 1) * (size_t)n, z));   // z = prec(r0) / prec(w)   (l.83-87)
    MG_TRY(dist_apply_A(h, L, MG_K_SPMV, z, w, nullptr));                    // w = A z                  (l.91)
    used = j + 1;
    for (int i = 0; i <= j; ++i) {                                           // t = AZ' * w              (l.95)
      double d = 0.0;
      MG_TRY(dist_dot(h, AZbuf.p + (size_t)i * (size_t)n, w, n, &d));
      Q.set(i, j, d);
    }
    MG_TRY(dist_dot(h, w, r0, n, &Q.xi[(size_t)j]));                         // xi[j] = dot(w, r0)       (l.97)
    const double rn = Q.step(rnorm0);                                        // t = pinv(H)*xi, ||r0 - AZ t||  (l.102-104)
    if (rn < TOL) break;                                                          // l.114-117
  }
  for (int j = 0; j < used; ++j)                                             // x0 += Z*t                (l.121-123)
    MG_TRY(dist_axpby(h, Q.t()[(size_t)j], Zbuf.p + (size_t)j * (size_t)L.cap_x, (j == 0 && x0_is_zero) ? 0.0 : 1.0, x0, n));
  return MG_OK;
}
}  // extern "C++"

// the sharded cycle: mirror of cycle_level (MGcycle.jl:1-118); returns the buffer holding x
// defer_post (optional, in/out): asked with true, the LAST post-smoothing sweep is left out where it can run fused with the
// residual that follows the cycle (dist_sweep_residual) - *defer_post tells whether it was.
int dist_cycle(mg_dist* h, int l, const double* b, double* xa, double* xb, bool x_zero, char ctype, double** result,
               bool r_valid = false, bool x1_ready = false, bool* defer_post = nullptr) {
  DistLevel& L = h->lev[(size_t)l];
  double *cur = xa, *alt = xb;
  long long npre = L.npre;
  const long long npost = L.npost;
  const double gmresTol = 1e-5;  // MGcycle.jl:5
  auto diag_prec = [&](const double* v, double* z) { return mg_vec_dscale_dev_FP64(L.d, v, z, L.n_own, h->nrhs, h->stream); };   // MM (l.36-38)
  if (h->relax_type == 1) {      // Jac-GMRES (MGcycle.jl:48-50): FGMRES on the residual, preconditioned by D
    const double* r0 = b;
    if (x_zero) {
      MG_TRY(dist_fill(h, cur, L.n_own, 0.0));
    } else {
      if (!r_valid) MG_TRY(dist_apply_A(h, L, MG_K_RESIDUAL, cur, L.r.p, b));
      r0 = L.r.p;
    }
    MG_TRY(dist_fgmres_relax(h, L, r0, cur, L.npre_raw, diag_prec, gmresTol, L.relZ, L.relAZ, false));
    npre = 0;
  } else if (x_zero) {
    MG_TRY(mg_vec_dscale_dev_FP64(L.d, b, cur, L.n_own, h->nrhs, h->stream));
    --npre;
  } else if (r_valid) {
    if (!x1_ready) MG_TRY(mg_vec_xpdr_dev_FP64(cur, L.d, L.r.p, alt, L.n_own, h->nrhs, h->stream));   // (else: written by the residual pass)
    std::swap(cur, alt);
    --npre;
  }
  // the last pre-smoothing sweep and the residual for the restriction as ONE pass where the level allows (MGcycle.jl:54-60)
  const bool pair_pre = npre >= 1 && dist_pair_ok(h, L, cur);
  for (long long s = 0; s < npre - (pair_pre ? 1 : 0); ++s) {
    MG_TRY(dist_apply_A(h, L, MG_K_SMOOTH, cur, alt, b));
    std::swap(cur, alt);
  }
  if (pair_pre && dist_pair_ok(h, L, cur)) {
    MG_TRY(dist_sweep_residual(h, L, cur, alt, L.r.p, nullptr, b, nullptr));
    std::swap(cur, alt);
  } else {
    if (pair_pre) {   // (the buffer the remaining sweep starts from is not aligned for the pass: two launches)
      MG_TRY(dist_apply_A(h, L, MG_K_SMOOTH, cur, alt, b));
      std::swap(cur, alt);
    }
    MG_TRY(dist_apply_A(h, L, MG_K_RESIDUAL, cur, L.r.p, b));
  }
  MG_TRY(dist_exchange_start(h, L.planR, L.r.p));
  // R held with the owned | halo column split: the coarse rows that read owned residuals only run beside the exchange
  auto restrict_to = [&](double* bc) {
    if (L.R && L.R->M.regular_cols >= 0) {
      MG_TRY(mg_op_apply_phase_dev_FP64(L.R, MG_K_RESTRICT, 1.0, L.r.p, 0.0, bc, nullptr, nullptr, h->nrhs, 0, 1, h->stream));
      MG_TRY(dist_exchange_finish(h, L.planR));
      MG_TRY(mg_op_apply_phase_dev_FP64(L.R, MG_K_RESTRICT, 1.0, L.r.p, 0.0, bc, nullptr, nullptr, h->nrhs, 0, 2, h->stream));
    } else {
      MG_TRY(dist_exchange_finish(h, L.planR));
      MG_TRY(dist_apply(h, L.R, MG_K_RESTRICT, 1.0, L.r.p, 0.0, bc, nullptr, nullptr, 0));
    }
    return (int)MG_OK;
  };
  if (l + 1 < (int)h->lev.size()) {
    DistLevel& C = h->lev[(size_t)l + 1];
    MG_TRY(restrict_to(C.b.p));
    double* xc = nullptr;
    if (ctype == 'K') {
      // K-cycle (MGcycle.jl:72-76): 2 steps of FGMRES on A_{l+1} xc = bc, preconditioned by the K-cycle of level l+1
      // (level l+1 is sharded, hence never the coarsest).  C.x0 doubles as scratch of the inner cycles (xc = 0 on entry).
      auto kprec = [&](const double* v, double* z) {
        double* res = nullptr;
        MG_TRY(dist_cycle(h, l + 1, v, C.x0.p, C.x1.p, true, 'K', &res));
        HIP_TRY(hipMemcpyAsync(z, res, sizeof(double) * (size_t)C.n_own, hipMemcpyDeviceToDevice, h->stream));
        return (int)MG_OK;
      };
      MG_TRY(dist_fgmres_relax(h, C, C.b.p, C.x0.p, 2, kprec, gmresTol, C.kZ, C.kAZ, true));
      xc = C.x0.p;
    } else {
      MG_TRY(dist_cycle(h, l + 1, C.b.p, C.x0.p, C.x1.p, true, ctype, &xc));
    }
    if (ctype == 'W' || ctype == 'F') {
      double* other = (xc == C.x0.p) ? C.x1.p : C.x0.p;
      MG_TRY(dist_cycle(h, l + 1, C.b.p, xc, other, false, ctype == 'W' ? 'W' : 'V', &xc));
    }
    MG_TRY(dist_exchange_start(h, L.planP, xc));
    if (L.P && L.P->M.regular_cols >= 0) {   // grid form: the rows that read owned coarse entries only run beside the exchange
      MG_TRY(mg_op_apply_phase_dev_FP64(L.P, MG_K_PROLONG, 1.0, xc, 1.0, cur, nullptr, nullptr, h->nrhs, 0, 1, h->stream));
      MG_TRY(dist_exchange_finish(h, L.planP));
      MG_TRY(mg_op_apply_phase_dev_FP64(L.P, MG_K_PROLONG, 1.0, xc, 1.0, cur, nullptr, nullptr, h->nrhs, 0, 2, h->stream));
    } else {
      MG_TRY(dist_exchange_finish(h, L.planP));
      MG_TRY(dist_apply(h, L.P, MG_K_PROLONG, 1.0, xc, 1.0, cur, nullptr, nullptr, 0));
    }
  } else {
    // restrict into this rank's rows of the first replicated level, all-gather, run the tail replicated
    MG_TRY(restrict_to(h->bc_pad.p));
    MG_TRY(h->T.allgather(h->bc_pad.p, h->bc_all.p, (size_t)(h->max_tail * h->nrhs), h->stream));   // (doubles per rank: padded share x right-hand sides)
    hipLaunchKernelGGL(dist_gather64, dim3((unsigned)((h->n_tail * h->nrhs + 255) / 256)), dim3(256), 0, h->stream, h->bc_all.p, h->gather_index.p, h->b_tail.p, h->n_tail, (int)h->nrhs);
    HIP_TRY(hipGetLastError());
    MG_TRY(mg_set_cycle_type(h->tail, ctype));
    if (ctype == 'K' && (long long)h->lev.size() < h->nl_total - 1) {
      // the first replicated level is not the coarsest: its K-step runs replicated, identically on every rank
      MG_TRY(mg_kcycle_step_async_dev_FP64(h->tail, h->b_tail.p, h->x_tail.p, h->n_tail));
    } else
    MG_TRY(mg_cycle_async_dev_FP64(h->tail, h->b_tail.p, h->x_tail.p, h->n_tail, h->nrhs, 1));
    if ((long long)h->lev.size() < h->nl_total - 1 && (ctype == 'W' || ctype == 'F')) {       // second visit (MGcycle.jl:79-84)
      MG_TRY(mg_set_cycle_type(h->tail, ctype == 'W' ? 'W' : 'V'));
      MG_TRY(mg_cycle_async_dev_FP64(h->tail, h->b_tail.p, h->x_tail.p, h->n_tail, h->nrhs, 0));
    }
    MG_TRY(dist_apply(h, L.P, MG_K_PROLONG, 1.0, h->x_tail.p, 1.0, cur, nullptr, nullptr, 0));
  }
  if (h->relax_type == 1) {      // MGcycle.jl:96-98
    MG_TRY(dist_apply_A(h, L, MG_K_RESIDUAL, cur, L.r.p, b));
    MG_TRY(dist_fgmres_relax(h, L, L.r.p, cur, L.npost_raw, diag_prec, gmresTol, L.relZ, L.relAZ, false));
  } else {
    const bool defer = defer_post && *defer_post && npost >= 1;
    for (long long s = 0; s < npost - (defer ? 1 : 0); ++s) {
      MG_TRY(dist_apply_A(h, L, MG_K_SMOOTH, cur, alt, b));
      std::swap(cur, alt);
    }
    if (defer_post) *defer_post = defer && dist_pair_ok(h, L, cur);
    if (defer && !*defer_post) {   // (not fusable from this buffer after all: the sweep runs here)
      MG_TRY(dist_apply_A(h, L, MG_K_SMOOTH, cur, alt, b));
      std::swap(cur, alt);
    }
  }
  if (h->relax_type == 1 && defer_post) *defer_post = false;
  *result = cur;
  return MG_OK;
}

int dist_set_plan(mg_dist* h, DistPlan& p, long long n_own_src, long long n_halo, long long n_send, const long long* send_idx,
                  const long long* send_splits, const long long* recv_splits, long long active) {
  p.set = true;
  p.active = active != 0;
  p.n_own_src = n_own_src;
  p.n_halo = n_halo;
  p.n_send = n_send;
  p.send_splits.assign(send_splits, send_splits + h->T.world);
  p.recv_splits.assign(recv_splits, recv_splits + h->T.world);
  long long ss = 0, rs = 0;
  for (int q = 0; q < h->T.world; ++q) { ss += p.send_splits[(size_t)q]; rs += p.recv_splits[(size_t)q]; }
  if (ss != n_send || rs != n_halo) return fail(MG_ERR_INVALID, "halo plan: splits do not add up (send %lld/%lld, recv %lld/%lld)", ss, n_send, rs, n_halo);
  std::vector<int> idx((size_t)std::max<long long>(n_send, 1), 0);
  for (long long i = 0; i < n_send; ++i) {
    if (send_idx[i] < 0 || send_idx[i] >= n_own_src) return fail(MG_ERR_INVALID, "halo plan: send index out of range");
    idx[(size_t)i] = (int)send_idx[i];
  }
  MG_TRY(p.send_idx.alloc(idx.size()));
  MG_TRY(p.send_buf.alloc(idx.size() * (size_t)h->nrhs));
  HIP_TRY(hipMemcpy(p.send_idx.p, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice));
  return MG_OK;
}
void dist_free_plan(DistPlan& p) {
  p.send_idx.release();
  p.send_buf.release();
}
}  // namespace

int mg_dist_unique_id(char* id128) {
  if (!id128) return fail(MG_ERR_INVALID, "null argument");
  if (!g_rccl.load()) return fail(MG_ERR_HIP, "librccl.so could not be loaded");
  Rccl::UniqueId u;
  NCCL_TRY(g_rccl.GetUniqueId(&u));
  std::memcpy(id128, u.internal, 128);
  return MG_OK;
}

int mg_dist_create(long long device_id, long long rank, long long world, const char* unique_id128, long long nlevels,
                   long long nl_total, long long cycleType, mg_dist** out) {
  if (!out) return fail(MG_ERR_INVALID, "out is null");
  *out = nullptr;
  if (world < 1 || rank < 0 || rank >= world || nlevels < 1 || nl_total <= nlevels)
    return fail(MG_ERR_INVALID, "bad rank/world/levels (%lld/%lld, %lld sharded of %lld)", rank, world, nlevels, nl_total);
  if (cycleType != 'V' && cycleType != 'W' && cycleType != 'F' && cycleType != 'K') return fail(MG_ERR_UNSUPPORTED, "the sharded cycle implements V, W, F and K");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (ndev <= 0) return fail(MG_ERR_HIP, "no HIP device visible: the multigrid cycle has no CPU fallback");
  if (device_id < 0 || device_id >= ndev) return fail(MG_ERR_INVALID, "device_id=%lld but %d devices visible", device_id, ndev);
  HIP_TRY(hipSetDevice((int)device_id));
  mg_dist* h = new mg_dist();
  h->device = (int)device_id;
  h->T.rank = (int)rank;
  h->T.world = (int)world;
  h->cycle = (char)cycleType;
  h->nl_total = nl_total;
  h->lev.resize((size_t)nlevels);
  if (const char* e = std::getenv("MG_DIST_NO_PAIR")) h->no_pair = e[0] == '1';   // (read once, here: nothing on the launch path reads the environment)
  auto bail = [&](int rc) { mg_dist_destroy(h); return rc; };
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_packed, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&h->ev_landed, hipEventDisableTiming) != hipSuccess ||
      h->partial.alloc(1024) != MG_OK || h->partial2.alloc(256) != MG_OK || h->scalar.alloc(1) != MG_OK || hipHostMalloc(reinterpret_cast<void**>(&h->h_scalar), sizeof(double)) != hipSuccess)
    return bail(fail(MG_ERR_HIP, "stream / event / scratch creation failed"));
  if (unique_id128) {
    const int rc = h->T.init_rccl(unique_id128);
    if (rc != MG_OK) return bail(rc);
  }
  *out = h;
  return MG_OK;
}

// Ranks of this handle's communicator AS RCCL REPORTS THEM (ncclCommCount); 0 when the handle uses the plug-in transport.
int mg_dist_comm_count(mg_dist* h, long long* count) {
  if (!h || !count) return fail(MG_ERR_INVALID, "null argument");
  return h->T.comm_count(count);
}

// Right-hand sides per call (default 1): blocks are row-major [n][nrhs] everywhere, as in mg_hierarchy (MGdef.jl:163-176: the
// reference is block-capable everywhere; one Frobenius stopping criterion for the block, SolveFuncs.jl:30).  Call it right
// after mg_dist_create - the plans, the tail and the level vectors are sized with it.  Blocks run the pointwise smoothers and
// the V / W / F cycles (the K-cycle's and Jac-GMRES's small systems are per right-hand side in the reference: refused here).
int mg_dist_set_nrhs(mg_dist* h, long long nrhs) {
  if (!h || nrhs < 1) return fail(MG_ERR_INVALID, "null handle or nrhs < 1");
  for (const DistLevel& L : h->lev)
    if (L.planA.set || L.n_own > 0) return fail(MG_ERR_STATE, "mg_dist_set_nrhs must precede the levels and plans");
  if (h->tail) return fail(MG_ERR_STATE, "mg_dist_set_nrhs must precede mg_dist_set_tail_INT64");
  if (nrhs > 1 && (h->cycle == 'K' || h->relax_type == 1)) return fail(MG_ERR_UNSUPPORTED, "blocks of right-hand sides: V, W, F cycles with pointwise smoothers");
  h->nrhs = nrhs;
  h->finalized = false;
  return MG_OK;
}

int mg_dist_set_exchange_plugin(mg_dist* h, mg_exchange_fn fn, void* user) {
  if (!h) return fail(MG_ERR_INVALID, "null argument");
  return h->T.set_plugin(fn, user);
}

int mg_dist_set_level(mg_dist* h, long long level, long long n_own, long long n_int, mg_operator* A_int, mg_operator* A_bnd,
                      mg_operator* P, mg_operator* R, const double* d_dev, long long relaxPre, long long relaxPost) {
  if (!h) return fail(MG_ERR_INVALID, "null handle");
  if (level < 1 || level > (long long)h->lev.size()) return fail(MG_ERR_INVALID, "bad level %lld", level);
  if (n_own < 1 || n_int < 0 || n_int > n_own || !P || !R || !d_dev || (n_int > 0 && !A_int) || (n_int < n_own && !A_bnd))
    return fail(MG_ERR_INVALID, "inconsistent level description");
  DistLevel& L = h->lev[(size_t)level - 1];
  L.n_own = n_own;
  L.n_int = n_int;
  L.A_int = A_int;
  L.A_bnd = A_bnd;
  L.P = P;
  L.R = R;
  L.d = d_dev;
  L.npre = std::max<long long>(1, relaxPre);      // relax() always updates once (MGcycle.jl:127-134)
  L.npost = std::max<long long>(1, relaxPost);
  L.npre_raw = relaxPre;
  L.npost_raw = relaxPost;
  L.box = false;
  h->finalized = false;
  return MG_OK;
}

// 0: pointwise smoothers (Jac / SPAI, the relaxPrec vectors), 1: Jac-GMRES (FGMRES_relaxation preconditioned by the
// relaxPrec vector; relaxPre/relaxPost are its inner dimensions).  The replicated tail carries its own setting.
int mg_dist_set_relax_type(mg_dist* h, long long relax_type) {
  if (!h) return fail(MG_ERR_INVALID, "null handle");
  if (relax_type != 0 && relax_type != 1) return fail(MG_ERR_INVALID, "relax_type must be 0 (pointwise) or 1 (Jac-GMRES)");
  h->relax_type = (int)relax_type;
  return MG_OK;
}

// Level `level` holds its A as ONE box operator (mg_op_create_box_FP64_INT64, passed as A_int with n_int = n_own).
int mg_dist_set_level_box(mg_dist* h, long long level, long long on) {
  if (!h) return fail(MG_ERR_INVALID, "null handle");
  if (level < 1 || level > (long long)h->lev.size()) return fail(MG_ERR_INVALID, "bad level %lld", level);
  h->lev[(size_t)level - 1].box = on != 0;
  return MG_OK;
}

int mg_dist_set_plan_INT64(mg_dist* h, long long level, long long which, long long n_own_src, long long n_halo, long long n_send,
                           const long long* send_idx, const long long* send_splits, const long long* recv_splits, long long active) {
  UploadFence upload_fence;
  if (!h) return fail(MG_ERR_INVALID, "null handle");
  if (level < 1 || level > (long long)h->lev.size() || which < 0 || which > 2) return fail(MG_ERR_INVALID, "bad (level, which)");
  if (!send_splits || !recv_splits || (n_send > 0 && !send_idx) || n_halo < 0 || n_send < 0) return fail(MG_ERR_INVALID, "bad plan arrays");
  (void)hipSetDevice(h->device);
  DistLevel& L = h->lev[(size_t)level - 1];
  DistPlan& p = which == MG_OP_A ? L.planA : (which == MG_OP_P ? L.planP : L.planR);
  dist_free_plan(p);
  h->finalized = false;
  return dist_set_plan(h, p, n_own_src, n_halo, n_send, send_idx, send_splits, recv_splits, active);
}

int mg_dist_set_tail_INT64(mg_dist* h, mg_hierarchy* tail, long long n_tail, long long own_tail, long long max_tail,
                           const long long* gather_index) {
  UploadFence upload_fence;
  if (!h || !tail || !gather_index || n_tail < 1 || max_tail < 1 || own_tail < 0 || own_tail > max_tail) return fail(MG_ERR_INVALID, "bad tail description");
  MG_CF64_UNSUPPORTED(tail);
  if (tail->coarse_dd) return fail(MG_ERR_UNSUPPORTED, "a hierarchy whose coarsest solve is a Schwarz sweep (mg_set_coarse_dd) is not served as the tail of a sharded one");
  (void)hipSetDevice(h->device);
  h->tail = tail;
  h->n_tail = n_tail;
  h->own_tail = own_tail;
  h->max_tail = max_tail;
  const size_t kk = (size_t)h->nrhs;
  MG_TRY(h->bc_pad.alloc((size_t)max_tail * kk));
  MG_TRY(h->bc_all.alloc((size_t)max_tail * (size_t)h->T.world * kk));
  MG_TRY(h->b_tail.alloc((size_t)n_tail * kk));
  MG_TRY(h->x_tail.alloc((size_t)n_tail * kk));
  if (tail->nrhs != h->nrhs) return fail(MG_ERR_INVALID, "the tail hierarchy is set up for %lld right-hand sides, the sequencer for %lld", tail->nrhs, h->nrhs);
  MG_TRY(h->gather_index.alloc((size_t)n_tail));
  for (long long i = 0; i < n_tail; ++i)
    if (gather_index[i] < 0 || gather_index[i] >= max_tail * h->T.world) return fail(MG_ERR_INVALID, "gather index out of range");
  HIP_TRY(hipMemset(h->bc_pad.p, 0, h->bc_pad.bytes()));
  HIP_TRY(hipMemset(h->x_tail.p, 0, h->x_tail.bytes()));
  HIP_TRY(hipMemcpy(h->gather_index.p, gather_index, (size_t)n_tail * sizeof(long long), hipMemcpyHostToDevice));
  // The tail enqueues on this sequencer's stream from now on.  Its own stream (if it owns one) is parked, not destroyed,
  // and comes back with mg_dist_release_tail / mg_dist_destroy - the handle stays usable by its owner afterwards.
  graphs_clear(tail);
  (void)spin_sync(tail->lane0.stream);
  h->tail_prev_stream = tail->lane0.stream;
  h->tail_prev_owns = tail->lane0.owns_stream;
  h->tail_prev_no_graph = tail->opt.no_graph;
  h->tail_borrowed = true;
  tail->lane0.stream = h->stream;
  tail->lane0.owns_stream = false;
  // Measured at world size 1 on 256^3 (bench.py --force-sharded-path): replaying the tail as a HIP graph between the
  // all-gather and the prolongation costs 40-80 us per step (0.98 -> 1.02-1.06 ms) where the single-GPU cycle gains 23:
  // off unless the tail's handle asks for it (mg_set_option(tail, "dist_tail_graph", 1) / MG_DIST_TAIL_GRAPH=1).
  if (!tail->opt.dist_tail_graph) tail->opt.no_graph = true;
  h->finalized = false;
  return MG_OK;
}

int mg_dist_finalize(mg_dist* h) {
  UploadFence upload_fence;
  if (!h) return fail(MG_ERR_INVALID, "null handle");
  (void)hipSetDevice(h->device);
  if (!h->tail) return fail(MG_ERR_STATE, "the replicated tail was not set");
  for (DistLevel& L : h->lev)   // relaxPrec from the class dictionary where the level's A allows it
    if (L.A_int && L.d && L.A_int->M.has_rc) {
      const long long nreg = L.A_int->M.regular_cols >= 0 ? L.A_int->M.regular_cols : L.A_int->M.n_rows;
      (void)hipDeviceSynchronize();
      MG_TRY(derive_class_d_csr(L.A_int->M, L.d, (size_t)nreg));
    }
  MG_TRY(h->T.ready());
  const int a = (int)h->lev.size();
  for (int l = 0; l < a; ++l) {
    DistLevel& L = h->lev[(size_t)l];
    if (L.n_own < 1) return fail(MG_ERR_STATE, "sharded level %d was not set", l + 1);
    if (!L.planA.set || !L.planR.set || (l + 1 < a && !L.planP.set)) return fail(MG_ERR_STATE, "halo plans of level %d are incomplete", l + 1);
    long long halo_x = L.planA.n_halo;
    if (l > 0 && h->lev[(size_t)l - 1].planP.set) halo_x = std::max(halo_x, h->lev[(size_t)l - 1].planP.n_halo);
    L.cap_x = L.n_own + halo_x;
    L.cap_r = L.n_own + L.planR.n_halo;
    MG_TRY(L.x0.alloc((size_t)(L.cap_x * h->nrhs)));
    MG_TRY(L.x1.alloc((size_t)(L.cap_x * h->nrhs)));
    MG_TRY(L.r.alloc((size_t)(L.cap_r * h->nrhs)));
    HIP_TRY(hipMemset(L.x0.p, 0, L.x0.bytes()));
    HIP_TRY(hipMemset(L.x1.p, 0, L.x1.bytes()));
    HIP_TRY(hipMemset(L.r.p, 0, L.r.bytes()));
    if (l > 0) {
      MG_TRY(L.b.alloc((size_t)(L.n_own * h->nrhs)));
      HIP_TRY(hipMemset(L.b.p, 0, L.b.bytes()));
    }
  }
  // one ||r||^2 partial per workgroup of the fused residual pass: at most one per 256 rows, + the exception rows' blocks
  {
    size_t need = (size_t)(2 * (h->lev[0].n_own / 256 + 2) + 1024);
    if (h->lev[0].A_int) {
      const Csr& M = h->lev[0].A_int->M;
      need = std::max(need, (size_t)std::max(M.blocks1(), M.nblocks) + (size_t)(M.rc_nexc + mgk::BLK - 1) / mgk::BLK + 2);
    }
    MG_TRY(h->partial.alloc(need));
  }
  h->finalized = true;
  return MG_OK;
}

int mg_dist_cycle_dev_FP64(mg_dist* h, const double* b_loc, double* x_loc, long long n_own, long long x_is_zero) {
  if (!h || !b_loc || !x_loc) return fail(MG_ERR_INVALID, "null argument");
  if (!h->finalized) return fail(MG_ERR_STATE, "mg_dist_finalize was not called");
  DistLevel& L = h->lev[0];
  if (n_own != L.n_own) return fail(MG_ERR_INVALID, "n_own=%lld but this rank owns %lld fine rows", n_own, L.n_own);
  (void)hipSetDevice(h->device);
  HIP_TRY(hipMemcpyAsync(L.x0.p, x_loc, sizeof(double) * (size_t)(n_own * h->nrhs), hipMemcpyDeviceToDevice, h->stream));
  double* res = nullptr;
  MG_TRY(dist_cycle(h, 0, b_loc, L.x0.p, L.x1.p, x_is_zero != 0, h->cycle, &res));
  HIP_TRY(hipMemcpyAsync(x_loc, res, sizeof(double) * (size_t)(n_own * h->nrhs), hipMemcpyDeviceToDevice, h->stream));
  HIP_TRY(spin_sync(h->stream));
  return MG_OK;
}

// solveMG (SolveFuncs.jl:3-39) on sharded vectors
int mg_dist_solve_dev_FP64(mg_dist* h, const double* b_loc, double* x_loc, long long n_own, double tol, long long maxIter,
                           long long* iters, double* resvec) {
  if (!h || !b_loc || !x_loc || maxIter < 0) return fail(MG_ERR_INVALID, "null argument or maxIter < 0");
  if (!h->finalized) return fail(MG_ERR_STATE, "mg_dist_finalize was not called");
  DistLevel& L = h->lev[0];
  if (n_own != L.n_own) return fail(MG_ERR_INVALID, "n_own=%lld but this rank owns %lld fine rows", n_own, L.n_own);
  (void)hipSetDevice(h->device);
  double *cur = L.x0.p, *alt = L.x1.p;
  HIP_TRY(hipMemcpyAsync(cur, x_loc, sizeof(double) * (size_t)(n_own * h->nrhs), hipMemcpyDeviceToDevice, h->stream));
  double xn = 0.0, res0 = 0.0, res = 0.0;
  MG_TRY(dist_norm(h, cur, n_own * h->nrhs, &xn));
  bool x_zero = (xn == 0.0);
  bool x1_ready = false;
  if (x_zero) {
    MG_TRY(dist_norm(h, b_loc, n_own * h->nrhs, &res0));
  } else {
    MG_TRY(dist_residual_norm(h, L, cur, b_loc, nullptr, &res0, &x1_ready));
  }
  if (resvec) resvec[0] = res0;
  long long it = 0;
  // Where the fine level's A allows, the last post-smoothing sweep is left out of the cycle and runs fused with the residual of
  // the stopping test (SolveFuncs.jl:26-30): x -> the iterate t, ||r||, and xn = t + d.*r, the next cycle's first update;
  // three buffers rotate (as solve_dev does on one GPU)
  double* spare = nullptr;
  bool fuse_post = false;
  if (h->relax_type == 0 && L.npost >= 1 && dist_pair_ok(h, L, cur)) {
    if (L.x2.n != (size_t)L.cap_x) {
      MG_TRY(L.x2.alloc((size_t)L.cap_x));
      HIP_TRY(hipMemsetAsync(L.x2.p, 0, L.x2.bytes(), h->stream));
    }
    spare = L.x2.p;
    fuse_post = dist_pair_ok(h, L, alt) && dist_pair_ok(h, L, spare);
  }
  for (long long count = 1; count <= maxIter; ++count) {
    double* out = nullptr;
    bool deferred = fuse_post;
    MG_TRY(dist_cycle(h, 0, b_loc, cur, alt, x_zero, h->cycle, &out, count > 1 || !x_zero, x1_ready, fuse_post ? &deferred : nullptr));
    if (out != cur) std::swap(cur, alt);
    x_zero = false;
    if (fuse_post && deferred) {
      // cur = x before the last sweep; alt <- the iterate; spare <- t + d.*r (not written on the last step)
      MG_TRY(dist_sweep_residual(h, L, cur, alt, nullptr, count < maxIter ? spare : nullptr, b_loc, &res));
      x1_ready = count < maxIter;
      double* freed = cur;
      cur = alt;
      alt = spare;
      spare = freed;
    } else {
      MG_TRY(dist_residual_norm(h, L, cur, b_loc, (count < maxIter && h->relax_type == 0) ? alt : nullptr, &res, &x1_ready));
    }
    ++it;
    if (resvec) resvec[it] = res;
    if (res / res0 < tol) break;
  }
  HIP_TRY(hipMemcpyAsync(x_loc, cur, sizeof(double) * (size_t)(n_own * h->nrhs), hipMemcpyDeviceToDevice, h->stream));
  HIP_TRY(spin_sync(h->stream));
  if (iters) *iters = it;
  return MG_OK;
}

// Hand the replicated tail's hierarchy back to its owner: its stream and graph option as they were before
// mg_dist_set_tail_INT64.  Call it BEFORE destroying the tail's handle when that happens first; mg_dist_destroy calls it
// otherwise.  The sequencer cannot cycle afterwards (mg_dist_set_tail_INT64 again to re-attach).
int mg_dist_release_tail(mg_dist* h) {
  if (!h) return fail(MG_ERR_INVALID, "null handle");
  if (h->tail && h->tail_borrowed) {
    (void)hipSetDevice(h->device);
    if (h->stream) (void)spin_sync(h->stream);
    graphs_clear(h->tail);
    h->tail->lane0.stream = h->tail_prev_stream;
    h->tail->lane0.owns_stream = h->tail_prev_owns;
    h->tail->opt.no_graph = h->tail_prev_no_graph;
  }
  h->tail = nullptr;
  h->tail_borrowed = false;
  h->finalized = false;
  return MG_OK;
}

int mg_dist_destroy(mg_dist* h) {
  if (!h) return MG_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)spin_sync(h->stream);
  if (h->side) (void)spin_sync(h->side);
  h->T.release();
  (void)mg_dist_release_tail(h);
  for (auto& L : h->lev) {
    dist_free_plan(L.planA);
    dist_free_plan(L.planR);
    dist_free_plan(L.planP);
    L.x0.release();
    L.x1.release();
    L.x2.release();
    L.r.release();
    L.b.release();
  }
  h->bc_pad.release();
  h->bc_all.release();
  h->b_tail.release();
  h->x_tail.release();
  h->gather_index.release();
  h->partial.release();
  h->partial2.release();
  h->scalar.release();
  h->kry.release();
  if (h->h_scalar) (void)hipHostFree(h->h_scalar);
  if (h->ev_packed) (void)hipEventDestroy(h->ev_packed);
  if (h->ev_landed) (void)hipEventDestroy(h->ev_landed);
  if (h->side) (void)hipStreamDestroy(h->side);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return MG_OK;
}

}  // extern "C"
