// mg_dist_krylov.inc - part of libmgvcycle.so's single translation unit (included by mgvcycle.hip behind mg_dist.inc; not compiled on its own).
// MG-preconditioned Krylov drivers on the HALO form of the sharded hierarchy (mg_dist_*): solveCG_MG / solveBiCGSTAB_MG / solveGMRES_MG
// (SolveFuncs.jl:74-133) for hierarchies of general CSR operators (SA-AMG: SAAMGWrapper.jl:61-73 enters through PCG and BiCGSTAB only).
// The algorithms, flags and resvec layouts are those of pcg_dev / bicgstab_dev / fgmres_core in mg_krylov.inc; FGMRES IS that file's
// fgmres_loop on the space DistFgmres, and every driver reports through KrylovReport (mg_krylov_host.hpp).  On this form
//   * a product with A is dist_apply_A on level 1: ONE halo exchange of its input, overlapped with the interior rows.  The inputs are the
//     cycle's own level-1 buffers (x0 / x1, cap_x long: the preconditioned vector is multiplied where the cycle left it) and PCG's p;
//   * the preconditioner is one dist_cycle from x = 0;
//   * a scalar is a sum over this rank's rows (one fused pass of mg_krvec.hpp, which also does the vector update due at that point) and an
//     all-reduce; the scalars due at the same point of an iteration share ONE all-reduce and ONE host read-back (up to 8), so that every
//     rank branches on the same bits.  All-reduces per iteration outside the cycle: PCG 2, BiCGSTAB 3, FGMRES 2 per inner step (inner <= 8).
// How the counts are reached is written down at each driver.
namespace {

// scalar elements in front of the 16-byte path of a pass over these vectors: 0 (all on a 16-byte boundary), 1 (all 8 bytes past one),
// n (mixed: the scalar path throughout)
int krv_head(const void* const* ptrs, int np, long long n, long long* head) {
  int odd = 0;
  for (int i = 0; i < np; ++i) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(ptrs[i]);
    if (!a || (a & 7)) return fail(MG_ERR_INVALID, "a vector of a fused pass is null or not 8-byte aligned");
    odd += (int)((a >> 3) & 1);
  }
  *head = odd == 0 ? 0 : (odd == np ? std::min<long long>(1, n) : n);
  return MG_OK;
}
// one pass + (ns > 0) the sums of its first ns scalars into out[0 .. ns)
template <class Op>
int krv_launch(const Op& op, long long n, const void* const* ptrs, int np, double* part, int ns, double* out, hipStream_t s) {
  if (n < 1) return fail(MG_ERR_INVALID, "a fused pass needs n >= 1");
  if (Op::NS > 0 && (!part || (ns > 0 && !out))) return fail(MG_ERR_INVALID, "a fused pass with sums needs its work space and output");
  long long head = 0;
  MG_TRY(krv_head(ptrs, np, n, &head));
  const int nb = mgkv::krv_grid(n);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(mgkv::krv_pass<Op>), dim3(nb), dim3(mgkv::KB), 0, s, op, n, head, part);
  if (Op::NS > 0 && ns > 0) hipLaunchKernelGGL(mgkv::krv_final, dim3(ns), dim3(mgkv::KB), 0, s, part, nb, out);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
template <class Op>
int krv_launch(const Op& op, long long n, std::initializer_list<const void*> ptrs, double* part, int ns, double* out, hipStream_t s) {
  return krv_launch(op, n, ptrs.begin(), (int)ptrs.size(), part, ns, out, s);
}
int krv_dots(int k, const double* const* xs, const double* const* ys, long long n, double* part, double* out, hipStream_t s) {
  if (k < 1 || k > mgkv::MAXS || !xs || !ys) return fail(MG_ERR_INVALID, "dots: 1 to %d pairs", mgkv::MAXS);
  if (n < 1 || !part || !out) return fail(MG_ERR_INVALID, "dots: bad arguments");
  mgkv::OpDots op;
  op.k = k;
  const void* ptrs[2 * mgkv::MAXS];
  for (int c = 0; c < mgkv::MAXS; ++c) {
    op.x[c] = xs[c < k ? c : 0];
    op.y[c] = ys[c < k ? c : 0];
    ptrs[2 * c] = op.x[c];
    ptrs[2 * c + 1] = op.y[c];
  }
  return krv_launch(op, n, ptrs, 2 * mgkv::MAXS, part, k, out, s);
}
// w -= sum_j h_j v_j over any number of vectors, 8 per pass; the last pass leaves ||w||^2 in out[0] when out is given
int krv_gs_update(int m, const double* hcoef, const double* const* vs, double* w, long long n, double* part, double* out, hipStream_t s) {
  for (int j0 = 0; j0 < m; j0 += mgkv::MAXS) {
    mgkv::OpGsUpdate op;
    op.m = std::min(mgkv::MAXS, m - j0);
    op.w = w;
    for (int j = 0; j < mgkv::MAXS; ++j) {
      op.h[j] = j < op.m ? hcoef[j0 + j] : 0.0;
      op.v[j] = vs[j0 + (j < op.m ? j : 0)];
    }
    const bool last = j0 + mgkv::MAXS >= m;
    const void* ptrs[mgkv::MAXS + 1];
    for (int j = 0; j < mgkv::MAXS; ++j) ptrs[j] = op.v[j];
    ptrs[mgkv::MAXS] = w;
    MG_TRY(krv_launch(op, n, ptrs, mgkv::MAXS + 1, part, (last && out) ? 1 : 0, out, s));
  }
  return MG_OK;
}

// ---- what the three drivers share ----
struct DistKry {
  mg_dist* h;
  DistLevel& L;
  DistKrylov& K;
  const long long n;
  explicit DistKry(mg_dist* h_) : h(h_), L(h_->lev[0]), K(h_->kry), n(h_->lev[0].n_own) {}
  double* part(int slot) { return K.part.p + (size_t)slot * mgkv::MAXB; }
  double* scal(int slot) { return K.scal.p + slot; }
  int ensure(size_t doubles) {
    if (K.part.n == 0) {
      MG_TRY(K.part.alloc((size_t)2 * mgkv::MAXS * mgkv::MAXB));
      MG_TRY(K.scal.alloc((size_t)mgkv::MAXS));
      HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&K.h_scal), sizeof(double) * mgkv::MAXS));
    }
    if (K.vec.n < doubles) MG_TRY(K.vec.alloc(doubles));
    return MG_OK;
  }
  template <class Op> int pass(const Op& op, std::initializer_list<const void*> ptrs, int slot = 0, int ns = Op::NS) {
    return krv_launch(op, n, ptrs, part(slot), ns, scal(slot), h->stream);
  }
  int dot1(const double* x, const double* y, int slot) { return krv_dots(1, &x, &y, n, part(slot), scal(slot), h->stream); }
  int dot2(const double* x0, const double* y0, const double* x1, const double* y1) {
    const double* xs[2] = {x0, x1};
    const double* ys[2] = {y0, y1};
    return krv_dots(2, xs, ys, n, part(0), scal(0), h->stream);
  }
  // the first `count` scalars summed over all ranks, on the host: one all-reduce, one read-back
  int reduce(int count, const double** out) {
    MG_TRY(h->T.allreduce_now(K.scal.p, (size_t)count, K.h_scal, h->stream));
    *out = K.h_scal;
    return MG_OK;
  }
  int copy(double* dst, const double* src) {
    HIP_TRY(hipMemcpyAsync(dst, src, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, h->stream));
    return MG_OK;
  }
  // z = M(v): one cycle from x = 0; *z is the level-1 buffer (cap_x long) the cycle left its result in
  int prec(const double* v, double** z) { return dist_cycle(h, 0, v, L.x0.p, L.x1.p, true, h->cycle, z); }
  // y = A x ; r = b - A x (x: cap_x long, its halo tail is filled here)
  int product(double* x, double* y) { return dist_apply_A(h, L, MG_K_SPMV, x, y, nullptr); }
  int residual(const double* b, const double* x_own, double* r) {
    MG_TRY(copy(L.x0.p, x_own));
    return dist_apply_A(h, L, MG_K_RESIDUAL, L.x0.p, r, b);
  }
  int zero(double* x) {                          // the b = 0 exit: zeros, stream drained (flag -9 is the driver's)
    MG_TRY(dist_fill(h, x, n, 0.0));
    HIP_TRY(spin_sync(h->stream));
    return MG_OK;
  }
};

int dist_krylov_ready(mg_dist* h, const double* b, double* x, long long n_own, long long maxIter) {
  if (!h || !b || !x || maxIter < 0) return fail(MG_ERR_INVALID, "null argument or maxIter < 0");
  if (!h->finalized) return fail(MG_ERR_STATE, "mg_dist_finalize was not called");
  if (h->nrhs != 1) return fail(MG_ERR_UNSUPPORTED, "the sharded Krylov drivers of the halo form take one right-hand side (this handle: %lld)", h->nrhs);
  if (n_own != h->lev[0].n_own) return fail(MG_ERR_INVALID, "n_own=%lld but this rank owns %lld fine rows", n_own, h->lev[0].n_own);
  (void)hipSetDevice(h->device);
  return MG_OK;
}

// KrylovMethods.cg as restated above pcg_dev.  Scalars per iteration and where they travel:
//   behind q = A p:      p'q, r'q, q'q                      (one pass over p, q, r; one all-reduce)
//   behind z = M(r):     z'r and the ||r||^2 that the update x += alpha p, r -= alpha q summed in its own pass   (one all-reduce)
// The stopping test sits BETWEEN the two, in front of the cycle.  It uses ||r - alpha q||^2 = r'r - 2 alpha r'q + alpha^2 q'q from the
// exact (all-reduced) r'r, r'q, q'q of this iteration - rounding error a few ulp of r'r, i.e. relative 1e-16 * r'r / ||r_new||^2 - so that no
// cycle is spent on a converged residual and no third all-reduce on the norm alone; the summed ||r||^2 replaces the entry of resvec when it
// arrives, and is all-reduced at once (a third all-reduce) where the recurrence cancels more than 8 digits.  alpha, beta, x, r, p are the
// textbook ones throughout.
int dist_pcg(mg_dist* h, const double* b, double* x, double tol, long long maxIter, long long* iters, long long* flag_out, double* resvec) {
  DistKry D(h);
  const long long n = D.n, cap = D.L.cap_x;
  MG_TRY(D.ensure((size_t)(2 * n + cap)));
  double* r = D.K.vec.p;
  double* q = r + n;
  double* p = q + n;          // cap_x long: multiplied by A
  const double* s = nullptr;
  MG_TRY(D.dot1(b, b, 0));
  MG_TRY(D.reduce(1, &s));
  const double nr0 = std::sqrt(s[0]);
  KrylovReport rep(iters, flag_out, resvec, nullptr);
  if (nr0 == 0.0) {
    MG_TRY(D.zero(x));
    return rep.finish(0, -9);
  }
  MG_TRY(D.residual(b, x, r));                                        // r = b - A(x)
  double* z = nullptr;
  MG_TRY(D.prec(r, &z));                                              // z = M(r)
  MG_TRY(D.dot2(r, z, r, r));
  MG_TRY(D.reduce(2, &s));
  double gamma = s[0], rr = s[1];
  MG_TRY(D.copy(p, z));
  long long it = 0, flag = -1;
  for (long long k = 1; k <= maxIter; ++k) {
    it = k;
    MG_TRY(D.product(p, q));                                          // q = A(p)
    MG_TRY(D.pass(mgkv::OpPcgDots{p, q, r}, {p, q, r}));
    MG_TRY(D.reduce(3, &s));
    const double pq = s[0], rq = s[1], qq = s[2];
    const double alpha = gamma / pq;
    if (std::isinf(alpha) || alpha < 0.0) { flag = -2; break; }
    MG_TRY(D.pass(mgkv::OpPcgUpdate{alpha, p, q, x, r}, {p, q, x, r}));   // x += alpha p ; r -= alpha q ; this rank's ||r||^2 -> scalar 0
    double rr_new = std::fma(alpha * alpha, qq, std::fma(-2.0 * alpha, rq, rr));
    bool summed = false;
    if (!(rr_new > 1e-8 * rr)) {                                      // (cancellation, or not a number: the summed norm itself)
      MG_TRY(D.reduce(1, &s));
      rr_new = s[0];
      summed = true;
    }
    double rel = std::sqrt(rr_new) / nr0;
    rep.set(k - 1, rel);
    if (rel <= tol) { flag = 0; break; }
    MG_TRY(D.prec(r, &z));                                            // z = M(r)
    double zr = 0.0;
    if (summed) {
      MG_TRY(D.dot1(z, r, 0));
      MG_TRY(D.reduce(1, &s));
      zr = s[0];
      rr = rr_new;
    } else {
      MG_TRY(D.dot1(z, r, 1));
      MG_TRY(D.reduce(2, &s));
      rr = s[0];
      zr = s[1];
      rep.set(k - 1, std::sqrt(rr) / nr0);
    }
    const double beta = zr / gamma;
    gamma = zr;
    MG_TRY(D.pass(mgkv::OpXpby{beta, z, p}, {z, p}));                 // p = z + beta p
  }
  HIP_TRY(spin_sync(h->stream));
  return rep.finish(it, flag);
}

// KrylovMethods.bicgstb (M1 = the cycle, M2 = identity) as restated above bicgstab_dev.  Scalars per iteration:
//   behind v = A phat:          rtld'v                                                  (one all-reduce)
//   behind t = A shat:          t's, t't and the ||s||^2 that s = r - alpha v summed    (one all-reduce)
//   behind the update of x, r:  ||r||^2 and rtld'r, the next iteration's rho            (one all-reduce)
// ||s||^2 travels behind the second cycle and product: the half-step exit (flag -3) is then taken one cycle and one product late - work
// the other exits never do, and x, the flag and resvec are the same - in exchange for one all-reduce less in every iteration.  The first
// rho is ||r0||^2 (rtld = r0).
int dist_bicgstab(mg_dist* h, const double* b, double* x, double tol, long long maxIter, long long* iters, long long* flag_out, double* resvec,
                  long long* nres) {
  DistKry D(h);
  const long long n = D.n;
  MG_TRY(D.ensure((size_t)(6 * n)));
  double* r = D.K.vec.p;        // residual, then s
  double* p = r + n;
  double* v = p + n;
  double* rtld = v + n;
  double* t = rtld + n;
  double* phat = t + n;
  const double* s = nullptr;
  MG_TRY(D.dot1(b, b, 0));
  MG_TRY(D.reduce(1, &s));
  const double bn = std::sqrt(s[0]);
  KrylovReport rep(iters, flag_out, resvec, nres);
  if (bn == 0.0) {
    MG_TRY(D.zero(x));
    return rep.finish(0, -9);
  }
  MG_TRY(D.residual(b, x, r));
  MG_TRY(D.dot1(r, r, 0));
  MG_TRY(D.reduce(1, &s));
  double rho = s[0], err = std::sqrt(s[0]) / bn;
  long long it = 0, flag = -1;
  rep.record(err);
  if (err < tol) {
    HIP_TRY(spin_sync(h->stream));
    return rep.finish(0, 0);
  }
  MG_TRY(D.copy(rtld, r));
  double omega = 1.0, alpha = 0.0, rho1 = 0.0;
  for (long long k = 1; k <= maxIter; ++k) {
    it = k;
    if (rho == 0.0) { flag = -2; break; }
    if (k > 1) {
      const double beta = (rho / rho1) * (alpha / omega);
      MG_TRY(D.pass(mgkv::OpBicgP{beta, omega, r, v, p}, {r, v, p}));    // p = r + beta (p - omega v)
    } else {
      MG_TRY(D.copy(p, r));
    }
    double* z = nullptr;
    MG_TRY(D.prec(p, &z));                                            // phat = M1(p)
    MG_TRY(D.product(z, v));                                          // v = A phat, multiplied where the cycle left it
    MG_TRY(D.copy(phat, z));
    MG_TRY(D.dot1(rtld, v, 0));
    MG_TRY(D.reduce(1, &s));
    alpha = rho / s[0];
    MG_TRY(D.pass(mgkv::OpBicgS{alpha, v, r}, {v, r}));               // s = r - alpha v (in r) ; this rank's ||s||^2 -> scalar 0
    MG_TRY(D.prec(r, &z));                                            // shat = M1(s)
    MG_TRY(D.product(z, t));                                          // t = A shat
    MG_TRY(D.pass(mgkv::OpBicgTS{t, r}, {t, r}, 1));                  // t's, t't -> scalars 1, 2
    MG_TRY(D.reduce(3, &s));
    const double sn = std::sqrt(s[0]) / bn, ts = s[1], tt = s[2];
    rep.record(sn);
    if (sn < tol) {                                                   // converged on the half step
      const double ma = -alpha;
      const double* vs[1] = {phat};
      MG_TRY(krv_gs_update(1, &ma, vs, x, n, D.part(0), nullptr, h->stream));   // x += alpha phat
      flag = -3;
      break;
    }
    omega = ts / tt;
    MG_TRY(D.pass(mgkv::OpBicgXR{alpha, omega, phat, z, t, rtld, x, r}, {phat, z, t, rtld, x, r}));   // x += alpha phat + omega shat ; r = s - omega t
    MG_TRY(D.reduce(2, &s));
    err = std::sqrt(s[0]) / bn;
    rep.record(err);
    if (err <= tol) { flag = 0; break; }
    if (omega == 0.0) { flag = -2; break; }
    rho1 = rho;
    rho = s[1];
  }
  HIP_TRY(spin_sync(h->stream));
  return rep.finish(it, flag);
}

// KrylovMethods.fgmres as restated above fgmres_core (precond 0).  The Arnoldi step orthogonalises w = A z against v_1 .. v_{i+1} with the
// i + 1 dots taken TOGETHER on the incoming w (one pass, one all-reduce per 8 of them) and the update w -= sum h_k v_k fused with ||w||^2
// (second all-reduce): 2 all-reduces per inner step for inner <= 8 where taking each dot behind the previous update costs i + 2.  The two
// orderings differ by the loss of orthogonality of v_1 .. v_{i+1} times rounding, far below the 1e-10 the drivers are held to.
struct DistFgmres {   // the space fgmres_loop (mg_krylov.inc) runs on
  DistKry& D;
  mg_dist* h;
  const long long n;
  const int m;
  const double* b;
  double* x;
  double *V, *Z, *r;                              // m+1 basis vectors, m preconditioned vectors, residual
  std::vector<double> hc;
  std::vector<const double*> vp, wp;
  DistFgmres(DistKry& D_, int m_, const double* b_, double* x_)
      : D(D_), h(D_.h), n(D_.n), m(m_), b(b_), x(x_), V(D_.K.vec.p), Z(V + (size_t)(m_ + 1) * n), r(Z + (size_t)m_ * n),
        hc((size_t)m_ + 1, 0.0), vp((size_t)m_ + 1, nullptr), wp((size_t)m_ + 1, nullptr) {}
  int norm(const double* v, double* out) {
    const double* s = nullptr;
    MG_TRY(D.dot1(v, v, 0));
    MG_TRY(D.reduce(1, &s));
    *out = std::sqrt(s[0]);
    return MG_OK;
  }
  int norm_b(double* out) { return norm(b, out); }
  int zero_x() { return dist_fill(h, x, n, 0.0); }
  int sync() {
    HIP_TRY(spin_sync(h->stream));
    return MG_OK;
  }
  int done() { return MG_OK; }
  int residual(double* rn) {
    MG_TRY(D.residual(b, x, r));
    return norm(r, rn);
  }
  int start_basis(double rn) { return D.pass(mgkv::OpScale{1.0 / rn, r, V}, {r, V}); }
  int arnoldi(int i, HessenbergLsq<double>& G) {
    const double* s = nullptr;
    double* vi = V + (size_t)i * n;
    double* w = V + (size_t)(i + 1) * n;
    double* z = nullptr;
    MG_TRY(D.prec(vi, &z));                                              // z = M(V[:,i])
    MG_TRY(D.product(z, w));                                             // w = A z
    MG_TRY(D.copy(Z + (size_t)i * n, z));
    for (int k = 0; k <= i; ++k) { vp[(size_t)k] = V + (size_t)k * n; wp[(size_t)k] = w; }
    for (int k0 = 0; k0 <= i; k0 += mgkv::MAXS) {                        // h_k = w'v_k
      const int cnt = std::min(mgkv::MAXS, i + 1 - k0);
      MG_TRY(krv_dots(cnt, wp.data() + k0, vp.data() + k0, n, D.part(0), D.scal(0), h->stream));
      MG_TRY(D.reduce(cnt, &s));
      for (int c = 0; c < cnt; ++c) hc[(size_t)(k0 + c)] = G.h(k0 + c, i) = s[c];
    }
    MG_TRY(krv_gs_update(i + 1, hc.data(), vp.data(), w, n, D.part(0), D.scal(0), h->stream));   // w -= sum h_k v_k ; ||w||^2
    MG_TRY(D.reduce(1, &s));
    const double wn = std::sqrt(s[0]);
    G.hsub(i) = wn;
    if (wn != 0.0) MG_TRY(D.pass(mgkv::OpScale{1.0 / wn, w, w}, {w}));
    return MG_OK;
  }
  int update_x(int used, const double* y) {
    for (int i = 0; i < used; ++i) { hc[(size_t)i] = -y[i]; vp[(size_t)i] = Z + (size_t)i * n; }
    if (used > 0) MG_TRY(krv_gs_update(used, hc.data(), vp.data(), x, n, D.part(0), nullptr, h->stream));
    return MG_OK;
  }
};
int dist_fgmres(mg_dist* h, const double* b, double* x, long long inner, double tol, long long maxIter, long long* iters, long long* flag_out,
                double* resvec, long long* nres) {
  if (inner < 1 || inner > 64) return fail(MG_ERR_INVALID, "inner must be in [1,64]");
  DistKry D(h);
  const int m = (int)inner;
  MG_TRY(D.ensure((size_t)D.n * (size_t)(2 * m + 2)));
  DistFgmres sp(D, m, b, x);
  KrylovReport rep(iters, flag_out, resvec, nres);
  return fgmres_loop<double>(sp, m, tol, maxIter, rep);
}
}  // namespace

extern "C" {
int mg_dist_pcg_dev_FP64(mg_dist* h, const double* b_loc, double* x_loc, long long n_own, double tol, long long maxIter, long long* iters,
                         long long* flag, double* resvec) {
  MG_TRY(dist_krylov_ready(h, b_loc, x_loc, n_own, maxIter));
  return dist_pcg(h, b_loc, x_loc, tol, maxIter, iters, flag, resvec);
}
int mg_dist_bicgstab_dev_FP64(mg_dist* h, const double* b_loc, double* x_loc, long long n_own, double tol, long long maxIter, long long* iters,
                              long long* flag, double* resvec, long long* nres) {
  MG_TRY(dist_krylov_ready(h, b_loc, x_loc, n_own, maxIter));
  return dist_bicgstab(h, b_loc, x_loc, tol, maxIter, iters, flag, resvec, nres);
}
int mg_dist_fgmres_dev_FP64(mg_dist* h, const double* b_loc, double* x_loc, long long n_own, long long inner, double tol, long long maxIter,
                            long long* iters, long long* flag, double* resvec, long long* nres) {
  MG_TRY(dist_krylov_ready(h, b_loc, x_loc, n_own, maxIter));
  return dist_fgmres(h, b_loc, x_loc, inner, tol, maxIter, iters, flag, resvec, nres);
}
// halo exchanges started and all-reduces entered by this rank since mg_dist_create (what the schedule really communicates)
int mg_dist_stats(mg_dist* h, long long* exchanges, long long* allreduces) {
  if (!h) return fail(MG_ERR_INVALID, "null handle");
  if (exchanges) *exchanges = h->T.n_exchanges;
  if (allreduces) *allreduces = h->T.n_allreduce;
  return MG_OK;
}

// ---- the fused passes on their own (tests, callers with Krylov loops of their own): asynchronous on `stream`; workspace_dev >= 8192
//      doubles, out_dev receives the pass's sums over the n elements ----
#define KRV_STREAM reinterpret_cast<hipStream_t>(stream)
int mg_vec_dots_dev_FP64(long long k, const double* const* xs_dev, const double* const* ys_dev, long long n, double* workspace_dev, double* out_dev,
                         void* stream) {
  return krv_dots((int)std::min<long long>(std::max<long long>(k, 0), mgkv::MAXS + 1), xs_dev, ys_dev, n, workspace_dev, out_dev, KRV_STREAM);
}
int mg_vec_pcg_dots_dev_FP64(const double* p, const double* q, const double* r, long long n, double* workspace_dev, double* out_dev, void* stream) {
  return krv_launch(mgkv::OpPcgDots{p, q, r}, n, {p, q, r}, workspace_dev, 3, out_dev, KRV_STREAM);
}
int mg_vec_pcg_update_dev_FP64(double alpha, const double* p, const double* q, double* x, double* r, long long n, double* workspace_dev,
                               double* out_dev, void* stream) {
  return krv_launch(mgkv::OpPcgUpdate{alpha, p, q, x, r}, n, {p, q, x, r}, workspace_dev, 1, out_dev, KRV_STREAM);
}
int mg_vec_xpby_dev_FP64(const double* x, double beta, double* y, long long n, void* stream) {
  return krv_launch(mgkv::OpXpby{beta, x, y}, n, {x, y}, nullptr, 0, nullptr, KRV_STREAM);
}
int mg_vec_scale_dev_FP64(double a, const double* x, double* y, long long n, void* stream) {
  return krv_launch(mgkv::OpScale{a, x, y}, n, {x, y}, nullptr, 0, nullptr, KRV_STREAM);
}
int mg_vec_bicg_p_dev_FP64(double beta, double omega, const double* r, const double* v, double* p, long long n, void* stream) {
  return krv_launch(mgkv::OpBicgP{beta, omega, r, v, p}, n, {r, v, p}, nullptr, 0, nullptr, KRV_STREAM);
}
int mg_vec_bicg_s_dev_FP64(double alpha, const double* v, double* r, long long n, double* workspace_dev, double* out_dev, void* stream) {
  return krv_launch(mgkv::OpBicgS{alpha, v, r}, n, {v, r}, workspace_dev, 1, out_dev, KRV_STREAM);
}
int mg_vec_bicg_ts_dev_FP64(const double* t, const double* s, long long n, double* workspace_dev, double* out_dev, void* stream) {
  return krv_launch(mgkv::OpBicgTS{t, s}, n, {t, s}, workspace_dev, 2, out_dev, KRV_STREAM);
}
int mg_vec_bicg_xr_dev_FP64(double alpha, double omega, const double* phat, const double* shat, const double* t, const double* rtld, double* x,
                            double* r, long long n, double* workspace_dev, double* out_dev, void* stream) {
  return krv_launch(mgkv::OpBicgXR{alpha, omega, phat, shat, t, rtld, x, r}, n, {phat, shat, t, rtld, x, r}, workspace_dev, 2, out_dev, KRV_STREAM);
}
int mg_vec_gs_update_dev_FP64(long long m, const double* h_host, const double* const* vs_dev, double* w, long long n, double* workspace_dev,
                              double* out_dev, void* stream) {
  if (m < 1 || m > 64 || !h_host || !vs_dev || !w || n < 1 || !workspace_dev) return fail(MG_ERR_INVALID, "gs_update: 1 to 64 vectors, non-null arguments");
  return krv_gs_update((int)m, h_host, vs_dev, w, n, workspace_dev, out_dev, KRV_STREAM);
}
#undef KRV_STREAM
}  // extern "C"
