// mg_complex_krylov.inc - part of libmgvcycle.so's single translation unit (included by mgvcycle.hip behind mg_complex.inc; not compiled on its own).
// ComplexF64 BiCGSTAB and FGMRES with one cycle of a CF64 hierarchy as preconditioner, vectors resident in HBM across iterations:
// solveBiCGSTAB_MG / solveGMRES_MG (SolveFuncs.jl:85-133) for VAL = ComplexF64 with an Afun of their own - the way Helmholtz problems
// are solved: the Krylov method runs on the (nearly) undamped operator, the hierarchy is built on a damped copy of it.
//   * The system operator is the handle's Krylov operator (mg_set_krylov_operator_CFP64_INT64; uploaded like As, conjugated once) or,
//     without one, As[1].  Products with it are cx_spmv<AXPBY> / <RESID>.
//   * The preconditioner is cx_cycle from x = 0 on the input vector.  Its result lives in lev[0].x[xi] and the next cycle overwrites
//     it, so it is COPIED OUT where it outlives the next cycle (BiCGSTAB's phat, FGMRES's Z_i; cx_cycle is left as it is); BiCGSTAB's
//     shat is consumed before the next cycle and is read where the cycle left it.
//   * BiCGSTAB is bicgstab_dev of mg_krylov.inc with complex scalars and conjugated dots (dot(a, b) = sum conj(a_i) b_i); FGMRES is
//     fgmres_loop of mg_krylov.inc itself, on the space CxFgmres with HessenbergLsq<std::complex<double>> (mg_krylov_host.hpp).  Flags,
//     stopping tests and the layout of resvec are theirs.  Every vector update and every scalar is one fused pass of mg_cxvec.hpp.
//   * Host synchronisations per iteration: BiCGSTAB 4 (dot(rtld, v) ; ||s|| ; (dot(t, s), dot(t, t)) ; (||r||, the next rho)), FGMRES 1 per
//     inner step (the chained Gram-Schmidt leaves the i + 2 scalars of a step in HBM; one readback).
//   * On a CF32 handle the drivers are the reference's mixed branch (VAL != eltype(B), SolveFuncs.jl:52-58): the system operator, every
//     Krylov vector, dot and scalar stay ComplexF64; only CxKry::prec changes - v is narrowed into the fine level's b, the single cycle
//     runs from zero, and the result is widened straight into phat / Z_i (the copy-out above, so no extra pass there) or into one more
//     work vector for BiCGSTAB's shat.  Without a Krylov operator, As[1] is widened once into K (cx_widen_K): the Krylov product is
//     never single.
// Also here: the stand-alone entry points of the passes (mg_cvec_*_dev_CFP64) and mg_cycle_dev_CFP64.
namespace {

typedef std::complex<double> zc;
inline cx_t cxv(zc a) { return cx_t{a.real(), a.imag()}; }
inline const cx_t* ccx(const double* p) { return reinterpret_cast<const cx_t*>(p); }
inline cx_t* mcx(double* p) { return reinterpret_cast<cx_t*>(p); }

// every vector of a complex pass starts on a 16-byte boundary
int cxv_aligned(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (!a || (a & 15)) return fail(MG_ERR_INVALID, "a vector of a complex pass is null or not 16-byte aligned");
  }
  return MG_OK;
}
// one pass + (ns > 0) the sums of its first ns scalars into out[0 .. ns)
template <class Op>
int cxv_launch(const Op& op, long long n, std::initializer_list<const void*> ptrs, double* part, int ns, double* out, hipStream_t s) {
  if (n < 1) return fail(MG_ERR_INVALID, "a complex pass needs n >= 1");
  if (Op::NS > 0 && (!part || (ns > 0 && !out))) return fail(MG_ERR_INVALID, "a complex pass with sums needs its work space and output");
  MG_TRY(cxv_aligned(ptrs));
  const int nb = mgcv::cxv_grid(n);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(mgcv::cxv_pass<Op>), dim3(nb), dim3(mgcv::KB), 0, s, op, n, part);
  if (Op::NS > 0 && ns > 0) hipLaunchKernelGGL(mgkv::krv_final, dim3(ns), dim3(mgcv::KB), 0, s, part, nb, out);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
// out[2c], out[2c+1] = dot(xs[c], ys[c]), c < k <= 4
int cxv_dots(int k, const double* const* xs, const double* const* ys, long long n, double* part, double* out, hipStream_t s) {
  if (k < 1 || k > mgcv::MAXD || !xs || !ys) return fail(MG_ERR_INVALID, "complex dots: 1 to %d pairs", mgcv::MAXD);
  if (!part || !out) return fail(MG_ERR_INVALID, "complex dots: null work space or output");
  mgcv::OpCDots op;
  op.k = k;
  for (int c = 0; c < mgcv::MAXD; ++c) {
    op.x[c] = ccx(xs[c < k ? c : 0]);
    op.y[c] = ccx(ys[c < k ? c : 0]);
  }
  return cxv_launch(op, n, {op.x[0], op.x[1], op.x[2], op.x[3], op.y[0], op.y[1], op.y[2], op.y[3]}, part, 2 * k, out, s);
}
// w -= sum_j h_j v_j over any number of vectors, 8 per pass; the last pass leaves ||w||^2 in out[0] when out is given.
// hcoef: m complex coefficients, interleaved.
int cxv_gs_update(int m, const double* hcoef, const double* const* vs, double* w, long long n, double* part, double* out, hipStream_t s) {
  for (int j0 = 0; j0 < m; j0 += mgcv::MAXV) {
    mgcv::OpCGsUpdate op;
    op.m = std::min(mgcv::MAXV, m - j0);
    op.w = mcx(w);
    for (int j = 0; j < mgcv::MAXV; ++j) {
      const int jj = j0 + (j < op.m ? j : 0);
      op.h[j] = j < op.m ? cx_t{hcoef[2 * jj], hcoef[2 * jj + 1]} : cx_t{0.0, 0.0};
      op.v[j] = ccx(vs[jj]);
    }
    const bool last = j0 + mgcv::MAXV >= m;
    MG_TRY(cxv_launch(op, n, {op.v[0], op.v[1], op.v[2], op.v[3], op.v[4], op.v[5], op.v[6], op.v[7], op.w}, part, (last && out) ? 1 : 0, out, s));
  }
  return MG_OK;
}

// ---- what the two drivers share ----
struct CxKry {
  mg_hierarchy* h;
  CxState& S;
  const long long n;
  const CxMat& A;      // the system operator
  hipStream_t st;
  explicit CxKry(mg_hierarchy* h_) : h(h_), S(*h_->cx), n(h_->cx->lev[0].n), A(h_->cx->K.set ? h_->cx->K : h_->cx->lev[0].A), st(h_->play->stream) {}
  double* part() { return S.kpart.p; }
  double* scal() { return S.kscal.p; }
  // work space: `vecs` complex vectors of n and the scalars' buffers, allocated at the first call and kept with the handle
  int ensure(size_t vecs) {
    if (S.kpart.n == 0) MG_TRY(S.kpart.alloc((size_t)mgcv::MAXS * mgcv::MAXB));
    if (S.kscal.n == 0) MG_TRY(S.kscal.alloc(CxState::KSCAL));
    if (!S.h_kscal) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&S.h_kscal), sizeof(double) * CxState::KSCAL));
    const size_t need = vecs * 2 * (size_t)n;
    if (S.kwork.n < need) MG_TRY(S.kwork.alloc(need));
    return MG_OK;
  }
  cx_t* vec(size_t i) { return cxp(S.kwork) + i * (size_t)n; }
  template <class Op> int pass(const Op& op, std::initializer_list<const void*> ptrs, int ns = Op::NS) {
    return cxv_launch(op, n, ptrs, part(), ns, scal(), st);
  }
  int dot1(const cx_t* x, const cx_t* y) {
    const double* xs[1] = {reinterpret_cast<const double*>(x)};
    const double* ys[1] = {reinterpret_cast<const double*>(y)};
    return cxv_dots(1, xs, ys, n, part(), scal(), st);
  }
  // the first `count` doubles of the scalar buffer on the host: one readback, one synchronisation
  int read(int count, const double** out) {
    HIP_TRY(hipMemcpyAsync(S.h_kscal, S.kscal.p, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, st));
    HIP_TRY(spin_sync(st));
    *out = S.h_kscal;
    return MG_OK;
  }
  int copy(cx_t* dst, const cx_t* src) {
    HIP_TRY(hipMemcpyAsync(dst, src, sizeof(cx_t) * (size_t)n, hipMemcpyDeviceToDevice, st));
    return MG_OK;
  }
  // *z = M(v): one cycle from x = 0; *z is the level buffer the cycle left its result in (valid until the next cycle)
  // On a CF32 handle (the reference's mixed closure, SolveFuncs.jl:52-58): v is narrowed into the fine level's b, the single cycle
  // runs from zero and its result is widened into `wide`, which *z then names.
  int prec(const cx_t* v, const cx_t** z, cx_t* wide = nullptr) {
    int xi = 0;
    CxLevel& L0 = S.lev[0];
    if (!S.single) {
      MG_TRY(cx_cycle<cx_t>(h, 0, v, xi, true, h->cycle));
      *z = cxp(L0.x[xi]);
      return MG_OK;
    }
    if (!wide) return fail(MG_ERR_INVALID, "internal: the mixed preconditioner needs a ComplexF64 vector for its result");
    MG_TRY(cx_narrow(h, v, cxp<cf_t>(L0.b), n));
    MG_TRY(cx_cycle<cf_t>(h, 0, cxc<cf_t>(L0.b), xi, true, h->cycle));
    MG_TRY(cx_widen(h, cxc<cf_t>(L0.x[xi]), wide, n));
    *z = wide;
    return MG_OK;
  }
  // dst = M(v), kept: the copy-out of the double cycle's result; the widening pass itself on a CF32 handle
  int prec_keep(const cx_t* v, cx_t* dst) {
    const cx_t* z = nullptr;
    MG_TRY(prec(v, &z, dst));
    return S.single ? MG_OK : copy(dst, z);
  }
  int product(const cx_t* x, cx_t* y) { return cx_spmv<mgk::AXPBY>(h, A, x, y, nullptr, nullptr, nullptr); }
  int residual(const cx_t* b, const cx_t* x, cx_t* r) { return cx_spmv<mgk::RESID>(h, A, x, r, b, nullptr, nullptr); }
  int zero(cx_t* x) {
    HIP_TRY(hipMemsetAsync(x, 0, sizeof(cx_t) * (size_t)n, st));
    return MG_OK;
  }
};

// bicgstab_dev (mg_krylov.inc) for complex vectors.  rho = dot(rtld, r), alpha = rho / dot(rtld, v), omega = dot(t, s) / dot(t, t),
// beta = (rho / rho1)(alpha / omega); breakdown is rho == 0 or omega == 0 as complex numbers.  The pass that ends an iteration
// (bicg_xr) also delivers dot(rtld, r) of the new r: the next iteration starts without a dot of its own.
int cx_bicgstab_dev(mg_hierarchy* h, const cx_t* b, cx_t* x, double tol, long long maxIter, long long* iters, long long* flag_out,
                    double* resvec, long long* nres) {
  CxKry K(h);
  MG_TRY(K.ensure(K.S.single ? 7 : 6));
  cx_t *r = K.vec(0), *p = K.vec(1), *v = K.vec(2), *rtld = K.vec(3), *t = K.vec(4), *phat = K.vec(5);
  cx_t* shat = K.S.single ? K.vec(6) : nullptr;   // (CF32: the widened s_hat; CF64: read where the cycle left it)
  const double* sc = nullptr;
  long long it = 0, flag = -1;
  KrylovReport rep(iters, flag_out, resvec, nres);
  MG_TRY(K.dot1(b, b));
  MG_TRY(K.read(1, &sc));
  const double bn = std::sqrt(sc[0]);
  if (bn == 0.0) {
    MG_TRY(K.zero(x));
    HIP_TRY(spin_sync(K.st));
    return rep.finish(0, -9);
  }
  MG_TRY(K.residual(b, x, r));
  MG_TRY(K.dot1(r, r));                               // ||r0||^2, and rho of the first iteration (rtld = r0)
  MG_TRY(K.read(2, &sc));
  double err = std::sqrt(sc[0]) / bn;
  zc rho(sc[0], sc[1]), rho1(0.0, 0.0), alpha(0.0, 0.0), omega(1.0, 0.0);
  rep.record(err);
  if (err < tol) return rep.finish(0, 0);
  MG_TRY(K.copy(rtld, r));
  for (long long k = 1; k <= maxIter; ++k) {
    it = k;
    if (rho == zc(0.0, 0.0)) { flag = -2; break; }
    if (k > 1) {
      const zc beta = (rho / rho1) * (alpha / omega);
      MG_TRY(K.pass(mgcv::OpCBicgP{cxv(beta), cxv(omega), r, v, p}, {r, v, p}));       // p = r + beta (p - omega v)
    } else {
      MG_TRY(K.copy(p, r));
    }
    const cx_t* z = nullptr;
    MG_TRY(K.prec_keep(p, phat));                                                       // p_hat = M1(p)
    MG_TRY(K.product(phat, v));
    MG_TRY(K.dot1(rtld, v));
    MG_TRY(K.read(2, &sc));                                                             // synchronisation 1
    alpha = rho / zc(sc[0], sc[1]);
    MG_TRY(K.pass(mgcv::OpCBicgS{cxv(alpha), v, r}, {v, r}));                           // s = r - alpha v (in r) ; ||s||^2
    MG_TRY(K.read(1, &sc));                                                             // synchronisation 2
    const double sn = std::sqrt(sc[0]) / bn;
    rep.record(sn);
    if (sn < tol) {                                                                     // converged on the half step
      const double ma[2] = {-alpha.real(), -alpha.imag()};
      const double* vs[1] = {reinterpret_cast<const double*>(phat)};
      MG_TRY(cxv_gs_update(1, ma, vs, reinterpret_cast<double*>(x), K.n, K.part(), nullptr, K.st));   // x += alpha p_hat
      flag = -3;
      break;
    }
    MG_TRY(K.prec(r, &z, shat));                                                            // s_hat = M1(s), read where the cycle left it
    MG_TRY(K.product(z, t));
    MG_TRY(K.pass(mgcv::OpCBicgTS{t, r}, {t, r}));
    MG_TRY(K.read(3, &sc));                                                             // synchronisation 3
    omega = zc(sc[0], sc[1]) / sc[2];
    MG_TRY(K.pass(mgcv::OpCBicgXR{cxv(alpha), cxv(omega), phat, z, t, rtld, x, r}, {phat, z, t, rtld, x, r}));
    MG_TRY(K.read(3, &sc));                                                             // synchronisation 4: ||r||^2 and the next rho
    err = std::sqrt(sc[0]) / bn;
    rep.record(err);
    if (err <= tol) { flag = 0; break; }
    if (omega == zc(0.0, 0.0)) { flag = -2; break; }
    rho1 = rho;
    rho = zc(sc[1], sc[2]);
  }
  HIP_TRY(spin_sync(K.st));
  return rep.finish(it, flag);
}

// The space fgmres_loop (mg_krylov.inc) runs on for complex vectors: H[k,i] = dot(V_k, w), H[i+1,i] = ||w|| (real); the rotations with
// a complex cosine and a real sine are HessenbergLsq<std::complex<double>> (mg_krylov_host.hpp).
struct CxFgmres {
  CxKry& K;
  const long long n;
  const int m;
  const cx_t* b;
  cx_t* x;
  cx_t *V, *Z, *r;                       // m+1 basis vectors, m preconditioned vectors, residual
  std::vector<double> ny;
  std::vector<const double*> zp;
  CxFgmres(CxKry& K_, int m_, const cx_t* b_, cx_t* x_)
      : K(K_), n(K_.n), m(m_), b(b_), x(x_), V(K_.vec(0)), Z(K_.vec((size_t)m_ + 1)), r(K_.vec((size_t)2 * m_ + 1)), ny((size_t)2 * m_), zp((size_t)m_) {
    for (int i = 0; i < m; ++i) zp[(size_t)i] = reinterpret_cast<const double*>(Z + (size_t)i * n);
  }
  int norm(const cx_t* v, double* out) {
    const double* sc = nullptr;
    MG_TRY(K.dot1(v, v));
    MG_TRY(K.read(1, &sc));
    *out = std::sqrt(sc[0]);
    return MG_OK;
  }
  int norm_b(double* out) { return norm(b, out); }
  int zero_x() { return K.zero(x); }
  int sync() {
    HIP_TRY(spin_sync(K.st));
    return MG_OK;
  }
  int done() { return MG_OK; }
  int residual(double* rn) {
    MG_TRY(K.residual(b, x, r));
    return norm(r, rn);
  }
  int start_basis(double rn) { return K.pass(mgcv::OpCScale{cx_t{1.0 / rn, 0.0}, r, V}, {r, V}); }
  int arnoldi(int i, HessenbergLsq<zc>& G) {
    const double* sc = nullptr;
    double* hd = K.scal();
    cx_t* vi = V + (size_t)i * n;
    cx_t* zi = Z + (size_t)i * n;
    cx_t* w = V + (size_t)(i + 1) * n;
    MG_TRY(K.prec_keep(vi, zi));                                                    // z = M(V[:,i])
    MG_TRY(K.product(zi, w));                                                       // w = A z
    // modified Gram-Schmidt as one chain on the device: h_k = dot(V_k, w) stays in HBM, the update w -= h_k V_k reads it there and
    // leaves the partials of the next dot (or of ||w||^2) in the same pass; the i + 2 scalars come back in ONE readback
    MG_TRY(K.dot1(V, w));
    for (int k = 0; k <= i; ++k) {
      const cx_t* vk = V + (size_t)k * n;
      const cx_t* u = k < i ? V + (size_t)(k + 1) * n : nullptr;
      MG_TRY(cxv_launch(mgcv::OpCMgsStep{hd + 2 * k, vk, u, w}, n, {vk, u ? u : vk, w}, K.part(), 2, hd + 2 * (k + 1), K.st));
    }
    MG_TRY(K.read(2 * (i + 2), &sc));
    for (int k = 0; k <= i; ++k) G.h(k, i) = zc(sc[2 * k], sc[2 * k + 1]);
    const double wn = std::sqrt(sc[2 * (i + 1)]);
    G.hsub(i) = wn;
    if (wn != 0.0) MG_TRY(K.pass(mgcv::OpCScale{cx_t{1.0 / wn, 0.0}, w, w}, {w}));  // V[:,i+1] = w/||w||
    return MG_OK;
  }
  int update_x(int used, const zc* y) {
    for (int i = 0; i < used; ++i) {
      ny[2 * (size_t)i] = -y[i].real();
      ny[2 * (size_t)i + 1] = -y[i].imag();
    }
    if (used > 0) MG_TRY(cxv_gs_update(used, ny.data(), zp.data(), reinterpret_cast<double*>(x), n, K.part(), nullptr, K.st));
    return MG_OK;
  }
};
int cx_fgmres_dev(mg_hierarchy* h, const cx_t* b, cx_t* x, long long inner, double tol, long long maxIter, long long* iters,
                  long long* flag_out, double* resvec, long long* nres) {
  const int m = (int)inner;
  CxKry K(h);
  MG_TRY(K.ensure((size_t)(2 * m + 2)));
  CxFgmres sp(K, m, b, x);
  KrylovReport rep(iters, flag_out, resvec, nres);
  return fgmres_loop<zc>(sp, m, tol, maxIter, rep);
}

// ---- blocks of right-hand sides: blockBiCGSTB (SolveFuncs.jl:94-96) for VAL = ComplexF64 ---------------------------------------------
// block_bicgstab_dev of mg_krylov.inc on complex blocks, row-major [n][k] ComplexF64 resident in HBM: products with the system operator
// are cx_csr_stream_spmm launches, the preconditioner is one block cycle from zero (on a CF32 handle the mixed closure on the whole
// block: narrow, the single cycle, widen), Gram matrices are X^H Y (one 16*k*k-byte readback each), the k x k solves run on the
// host (SmallMatT<zc>, mg_krylov_host.hpp), omega = tr(T^H S) / tr(T^H T).  Flags, resvec and the stopping tests are the real driver's.
typedef SmallMatT<zc> CMat;
struct CxBlkKry {
  mg_hierarchy* h;
  CxState& S;
  const long long n;
  const int k;
  const CxMat& A;      // the system operator
  hipStream_t st;
  static constexpr size_t SLOT = (size_t)mgk::BLK_KMAX * mgk::BLK_KMAX;   // complex entries of one coefficient matrix
  CxBlkKry(mg_hierarchy* h_, int k_) : h(h_), S(*h_->cx), n(h_->cx->lev[0].n), k(k_), A(h_->cx->K.set ? h_->cx->K : h_->cx->lev[0].A), st(h_->play->stream) {}
  size_t len() const { return (size_t)n * (size_t)k; }
  int nblocks() const { return (int)std::min<long long>(256, std::max<long long>(1, (n + mgk::BLK - 1) / mgk::BLK)); }
  int ensure(size_t blocks) {
    const size_t need = blocks * 2 * len(), gneed = 2 * ((size_t)nblocks() + 1) * SLOT;
    if (S.Bkwork.n < need) MG_TRY(S.Bkwork.alloc(need));
    if (S.Bgpart.n < gneed) MG_TRY(S.Bgpart.alloc(gneed));
    if (S.Bcoef.n == 0) MG_TRY(S.Bcoef.alloc(2 * SLOT * 8));
    if (!S.h_bgram) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&S.h_bgram), sizeof(double) * 2 * SLOT));
    if (!S.h_bcoef) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&S.h_bcoef), sizeof(double) * 2 * SLOT * 8));
    return MG_OK;
  }
  cx_t* blk(size_t i) { return cxp(S.Bkwork) + i * len(); }
  // the k x k matrix the partials of nb workgroups add up to (cx_blk_gram_final: workgroup order), on the host; synchronises the stream
  // (wave: block FGMRES's final kernel, one wavefront per entry - another fixed order, so block BiCGSTAB keeps the one it had)
  int gram_read(int nb, CMat& G, bool wave = false) {
    cx_t* part = cxp(S.Bgpart);
    cx_t* out = part + (size_t)nb * k * k;
    if (wave) hipLaunchKernelGGL(mgk::cx_blk_gram_final_wave, dim3(k * k), dim3(64), 0, st, part, nb, k, out);
    else hipLaunchKernelGGL(mgk::cx_blk_gram_final, dim3(1), dim3(mgk::BLK), 0, st, part, nb, k, out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(S.h_bgram, out, sizeof(cx_t) * k * k, hipMemcpyDeviceToHost, st));
    HIP_TRY(spin_sync(st));
    G = CMat(k, k);
    for (int e = 0; e < k * k; ++e) G.a[(size_t)e] = zc(S.h_bgram[2 * e], S.h_bgram[2 * e + 1]);
    return MG_OK;
  }
  // G = X^H Y to the host; synchronises the stream
  int gram(const cx_t* X, const cx_t* Y, CMat& G) {
    const int nb = nblocks();
    hipLaunchKernelGGL(mgk::cx_blk_gram_partial, dim3(nb, k), dim3(mgk::BLK), 0, st, X, Y, n, k, cxp(S.Bgpart));
    return gram_read(nb, G);
  }
  // the next of the ring of 8 coefficient slots, Cm on its way into it; the ring is drained once per lap (blk_comb)
  int coef(const CMat& Cm, cx_t** slot_out) {
    const unsigned si = S.bcoef_next++ % 8;
    if (si == 0 && S.bcoef_next > 1) HIP_TRY(spin_sync(st));
    double* hs = S.h_bcoef + 2 * SLOT * si;
    cx_t* slot = cxp(S.Bcoef) + SLOT * si;
    for (int e = 0; e < k * k; ++e) {
      hs[2 * e] = Cm.a[(size_t)e].real();
      hs[2 * e + 1] = Cm.a[(size_t)e].imag();
    }
    HIP_TRY(hipMemcpyAsync(slot, hs, sizeof(cx_t) * k * k, hipMemcpyHostToDevice, st));
    *slot_out = slot;
    return MG_OK;
  }
  // out = s*add + in*Cm (add may be null; out may alias in or add)
  int comb(cx_t* out, const cx_t* add, zc s, const cx_t* in, const CMat& Cm) {
    cx_t* slot = nullptr;
    MG_TRY(coef(Cm, &slot));
    hipLaunchKernelGGL(mgk::cx_blk_comb, dim3(cx_grid(n)), dim3(mgk::BLK), 0, st, out, add, cxv(s), in, slot, n, k);
    HIP_TRY(hipGetLastError());
    return MG_OK;
  }
  // ---- block FGMRES: every element of a Gram operand read once (cx_blk_gram_onepass), and the combination whose epilogue leaves
  //      the next Gram matrix (cx_blk_comb_gram); up to GRAM_WGS workgroups, several per CU, whose partials need a larger Bgpart
  //      than gram()'s (ensure_gram) ----
  static constexpr int GRAM_WGS = 1024;
  int ensure_gram() {
    const size_t gneed = 2 * ((size_t)GRAM_WGS + 1) * SLOT;
    if (S.Bgpart.n < gneed) MG_TRY(S.Bgpart.alloc(gneed));
    return MG_OK;
  }
  int lgk() const {
    int l = 0;
    while ((1 << l) < k) ++l;
    return l;
  }
  int gram_onepass(const cx_t* X, const cx_t* Y, CMat& G) {
    const long long tr = mgk::GRAM_TILE >> lgk();
    const int nb = (int)std::min<long long>(GRAM_WGS, (n + tr - 1) / tr);
    hipLaunchKernelGGL(mgk::cx_blk_gram_onepass, dim3(nb), dim3(mgk::BLK), 0, st, X, Y, n, k, lgk(), cxp(S.Bgpart));
    return gram_read(nb, G, true);
  }
  // out = s*add + in*Cm as comb, and G = Q^H out to the host (Q == out, or a block apart from the others); synchronises the stream
  // Above 8 columns the fused kernel measured slower than the two launches (profiles/complex_block_fgmres.md: 0.99 ms against
  // 0.57 + 0.26 ms at 16 columns; level at 8, ahead at 4 and 2), so there the update and the one-pass Gram matrix stay apart.
  int comb_gram(cx_t* out, const cx_t* add, zc s, const cx_t* in, const CMat& Cm, const cx_t* Q, CMat& G) {
    if (k > 8) {
      MG_TRY(comb(out, add, s, in, Cm));
      return gram_onepass(Q, out, G);
    }
    cx_t* slot = nullptr;
    MG_TRY(coef(Cm, &slot));
    const int nb = (int)std::min<long long>(GRAM_WGS, (n + mgk::BLK - 1) / mgk::BLK);
    hipLaunchKernelGGL(mgk::cx_blk_comb_gram, dim3(nb), dim3(mgk::BLK), 0, st, out, add, cxv(s), in, slot, Q, n, k, lgk(), cxp(S.Bgpart));
    return gram_read(nb, G, true);
  }
  // W -> an orthonormal block in place by Cholesky QR applied twice, Rf with W_in = Q Rf (blk_cholqr); G1: W^H W where the caller
  // has it already.  The second Gram matrix is the epilogue of the first scaling.
  int cholqr(cx_t* W, const CMat* G1, CMat& Rf) {
    CMat G;
    if (G1) G = *G1;
    else MG_TRY(gram_onepass(W, W, G));
    const CMat R1 = sm_chol_semidefinite(G);
    MG_TRY(comb_gram(W, nullptr, zc(0.0, 0.0), W, sm_tri_pinv(R1), W, G));
    const CMat R2 = sm_chol_semidefinite(G);
    MG_TRY(comb(W, nullptr, zc(0.0, 0.0), W, sm_tri_pinv(R2)));
    Rf = sm_mul(R2, R1);
    return MG_OK;
  }
  int colnorms(const cx_t* X, std::vector<double>& out) {
    CMat G;
    MG_TRY(gram(X, X, G));
    out.assign((size_t)k, 0.0);
    for (int j = 0; j < k; ++j) out[(size_t)j] = std::sqrt(std::max(0.0, G(j, j).real()));
    return MG_OK;
  }
  int copy(cx_t* dst, const cx_t* src) {
    HIP_TRY(hipMemcpyAsync(dst, src, sizeof(cx_t) * len(), hipMemcpyDeviceToDevice, st));
    return MG_OK;
  }
  // Z = M(V): one block cycle from zero, copied (CF64) or widened (CF32) out of the level buffer into Z
  int prec(const cx_t* V, cx_t* Z) {
    int xi = 0;
    CxLevel& L0 = S.lev[0];
    if (!S.single) {
      MG_TRY(cx_cycle<cx_t>(h, 0, V, xi, true, h->cycle, k));
      return copy(Z, cxc(L0.Bx[xi]));
    }
    MG_TRY(cx_narrow(h, V, cxp<cf_t>(L0.Bb), (long long)len()));
    MG_TRY(cx_cycle<cf_t>(h, 0, cxc<cf_t>(L0.Bb), xi, true, h->cycle, k));
    return cx_widen(h, cxc<cf_t>(L0.Bx[xi]), Z, (long long)len());
  }
  int product(const cx_t* X, cx_t* Y) { return cx_spmv<mgk::AXPBY>(h, A, X, Y, nullptr, nullptr, nullptr, cx_t{1, 0}, cx_t{0, 0}, k); }
  int residual(const cx_t* B, const cx_t* X, cx_t* R) { return cx_spmv<mgk::RESID>(h, A, X, R, B, nullptr, nullptr, cx_t{1, 0}, cx_t{0, 0}, k); }
};

int cx_block_bicgstab_dev(mg_hierarchy* h, const cx_t* B, cx_t* X, int k, double tol, long long maxIter, long long* iters,
                          long long* flag_out, double* resvec, long long* nres) {
  CxBlkKry K(h, k);
  MG_TRY(K.ensure(7));
  cx_t *R = K.blk(0), *R0 = K.blk(1), *P = K.blk(2), *Ph = K.blk(3), *V = K.blk(4), *Sh = K.blk(5), *T = K.blk(6);
  std::vector<double> nb, rn;
  MG_TRY(K.colnorms(B, nb));
  long long it = 0, flag = -1;
  KrylovReport rep(iters, flag_out, resvec, nres);
  bool any = false;
  for (double v : nb) any = any || v > 0.0;
  if (!any) {
    HIP_TRY(hipMemsetAsync(X, 0, sizeof(cx_t) * K.len(), K.st));
    HIP_TRY(spin_sync(K.st));
    return rep.finish(0, -9);
  }
  for (double& v : nb) if (!(v > 0.0)) v = 1.0;
  auto worst_rel = [&](const cx_t* blk, double* out) -> int {
    MG_TRY(K.colnorms(blk, rn));
    double wv = 0.0;
    for (int j = 0; j < k; ++j) wv = std::max(wv, rn[(size_t)j] / nb[(size_t)j]);
    *out = wv;
    return MG_OK;
  };
  const zc one(1.0, 0.0);
  MG_TRY(K.residual(B, X, R));
  double err = 0.0;
  MG_TRY(worst_rel(R, &err));
  rep.record(err);
  if (err < tol) return rep.finish(0, 0);
  MG_TRY(K.copy(R0, R));
  MG_TRY(K.copy(P, R));
  for (long long iter = 1; iter <= maxIter; ++iter) {
    it = iter;
    MG_TRY(K.prec(P, Ph));                                        // Phat = M(P)
    MG_TRY(K.product(Ph, V));                                     // V = A Phat
    CMat RtV, RtR, alpha;
    MG_TRY(K.gram(R0, V, RtV));
    MG_TRY(K.gram(R0, R, RtR));
    if (!sm_solve(RtV, RtR, alpha)) { flag = -2; break; }
    CMat nalpha = alpha;
    for (zc& v : nalpha.a) v = -v;
    MG_TRY(K.comb(R, R, one, V, nalpha));                         // S = R - V alpha   (in R)
    double sn = 0.0;
    MG_TRY(worst_rel(R, &sn));
    rep.record(sn);
    if (sn < tol) {
      MG_TRY(K.comb(X, X, one, Ph, alpha));
      flag = -3;
      break;
    }
    MG_TRY(K.prec(R, Sh));                                        // Shat = M(S)
    MG_TRY(K.product(Sh, T));                                     // T = A Shat
    CMat TS, TT;
    MG_TRY(K.gram(T, R, TS));
    MG_TRY(K.gram(T, T, TT));
    zc ts(0.0, 0.0);
    double tt = 0.0;
    for (int j = 0; j < k; ++j) { ts += TS(j, j); tt += TT(j, j).real(); }
    if (tt == 0.0) { flag = -2; break; }
    const zc omega = ts / tt;                                     // tr(T^H S) / tr(T^H T)
    MG_TRY(K.comb(X, X, one, Ph, alpha));                         // X += Phat alpha + omega Shat
    MG_TRY(K.comb(X, X, one, Sh, sm_scaled_identity(k, omega)));
    MG_TRY(K.comb(R, R, one, T, sm_scaled_identity(k, -omega)));  // R = S - omega T
    MG_TRY(worst_rel(R, &err));
    rep.record(err);
    if (err <= tol) { flag = 0; break; }
    if (omega == zc(0.0, 0.0)) { flag = -2; break; }
    CMat RtT, beta;
    MG_TRY(K.gram(R0, T, RtT));
    if (!sm_solve(RtV, RtT, beta)) { flag = -2; break; }
    for (zc& v : beta.a) v = -v;
    MG_TRY(K.comb(P, P, one, V, sm_scaled_identity(k, -omega)));  // P - omega V
    MG_TRY(K.comb(P, R, one, P, beta));                           // P = R + (P - omega V) beta
  }
  HIP_TRY(spin_sync(K.st));
  return rep.finish(it, flag);
}

// blockFGMRES (SolveFuncs.jl:130) for VAL = ComplexF64: block_fgmres_core of mg_krylov.inc line by line on complex blocks.
// V_0 = cholqr2(R), xi[:k] = Rf; per inner step Z_j = M(V_j), W = A Z_j, block modified Gram-Schmidt against V_0 .. V_j with
// H_ij = V_i^H W, cholqr2(W), the exact block least squares on the host (sm_lstsq on SmallMatT<zc>) and the estimate
// ||xi - H Y||_F / ||B||_F; X += sum Z_j Y_j; the true residual at a restart.  Work set: 2*inner + 2 blocks (V: inner + 1, Z: inner, R).
// Gram matrices: H_0j free-standing (cx_blk_gram_onepass); H_{i+1,j} is the epilogue of W -= V_i H_ij, W^H W that of the last update,
// and the second Gram matrix of cholqr2 that of its first scaling (cx_blk_comb_gram) - j + 3 per inner step, one host
// synchronisation each (above 8 columns the epilogues are launches of cx_blk_gram_onepass behind cx_blk_comb, see comb_gram).  At a
// restart R^H R serves both ||R||_F and the first factor of cholqr2(R).
int cx_block_fgmres_dev(mg_hierarchy* h, const cx_t* B, cx_t* X, int k, long long inner, double tol, long long maxIter, long long* iters,
                        long long* flag_out, double* resvec, long long* nres) {
  CxBlkKry K(h, k);
  const int m = (int)inner;
  MG_TRY(K.ensure((size_t)(2 * m + 2)));
  MG_TRY(K.ensure_gram());
  const size_t len = K.len();
  cx_t* Vb = K.blk(0);                       // m+1 blocks
  cx_t* Zb = K.blk((size_t)m + 1);           // m blocks
  cx_t* R = K.blk((size_t)2 * m + 1);        // residual
  long long flag = -1, total = 0;
  KrylovReport rep(iters, flag_out, resvec, nres);
  CMat GR;
  auto fro = [&](const cx_t* blk, double* out) -> int {   // ||blk||_F from the diagonal of blk^H blk, which stays in GR
    MG_TRY(K.gram_onepass(blk, blk, GR));
    double s2 = 0.0;
    for (int j = 0; j < k; ++j) {
      const double cn = std::sqrt(std::max(0.0, GR(j, j).real()));
      s2 += cn * cn;
    }
    *out = std::sqrt(s2);
    return MG_OK;
  };
  const zc one(1.0, 0.0);
  double bn = 0.0, rn = 0.0;
  MG_TRY(fro(B, &bn));
  if (bn == 0.0) {
    HIP_TRY(hipMemsetAsync(X, 0, sizeof(cx_t) * len, K.st));
    HIP_TRY(spin_sync(K.st));
    return rep.finish(0, -9);
  }
  MG_TRY(K.residual(B, X, R));
  MG_TRY(fro(R, &rn));
  if (rn / bn < tol) return rep.finish(0, 0);
  for (long long it = 1; it <= maxIter && flag != 0; ++it) {
    CMat H((m + 1) * k, m * k), xi((m + 1) * k, k), Rf, Y;
    MG_TRY(K.copy(Vb, R));
    MG_TRY(K.cholqr(Vb, &GR, Rf));                                 // (GR = R^H R, left by fro(R))
    for (int i = 0; i < k; ++i)
      for (int j = 0; j < k; ++j) xi(i, j) = Rf(i, j);
    int used = 0;
    for (int j = 0; j < m; ++j) {
      cx_t* Vj = Vb + (size_t)j * len;
      cx_t* Zj = Zb + (size_t)j * len;
      cx_t* W = Vb + (size_t)(j + 1) * len;
      MG_TRY(K.prec(Vj, Zj));                                      // Z_j = M(V_j)
      MG_TRY(K.product(Zj, W));                                    // W = A Z_j
      CMat Hij, Gn;
      MG_TRY(K.gram_onepass(Vb, W, Hij));                          // H_0j = V_0^H W
      for (int i = 0; i <= j; ++i) {                               // block modified Gram-Schmidt
        for (int a = 0; a < k; ++a)
          for (int b = 0; b < k; ++b) H(i * k + a, j * k + b) = Hij(a, b);
        for (zc& v : Hij.a) v = -v;
        const cx_t* Vi = Vb + (size_t)i * len;
        MG_TRY(K.comb_gram(W, W, one, Vi, Hij, i < j ? Vi + len : W, Gn));   // W -= V_i H_ij ; V_{i+1}^H W, at the end W^H W
        Hij = Gn;
      }
      CMat Hn;
      MG_TRY(K.cholqr(W, &Hij, Hn));
      for (int a = 0; a < k; ++a)
        for (int b = 0; b < k; ++b) H((j + 1) * k + a, j * k + b) = Hn(a, b);
      CMat Hb((j + 2) * k, (j + 1) * k), xb((j + 2) * k, k);
      for (int a = 0; a < Hb.r; ++a) {
        for (int b = 0; b < Hb.c; ++b) Hb(a, b) = H(a, b);
        for (int b = 0; b < k; ++b) xb(a, b) = xi(a, b);
      }
      const double err = sm_lstsq(Hb, xb, Y) / bn;
      rep.record(err);
      ++total;
      used = j + 1;
      if (err <= tol) { flag = 0; break; }
    }
    for (int j = 0; j < used; ++j) {                               // X += Z_j Y_j
      CMat Yj(k, k);
      for (int a = 0; a < k; ++a)
        for (int b = 0; b < k; ++b) Yj(a, b) = Y(j * k + a, b);
      MG_TRY(K.comb(X, X, one, Zb + (size_t)j * len, Yj));
    }
    if (flag == 0) break;
    MG_TRY(K.residual(B, X, R));
    MG_TRY(fro(R, &rn));
    if (rn / bn <= tol) { flag = 0; break; }
  }
  HIP_TRY(spin_sync(K.st));
  return rep.finish(total, flag);
}

// The checks every driver entry point shares, vector (W.nr == 0) or block.  device_form: b, x resident (a block: row-major [n][nrhs]);
// host form: staged through the work set's staging buffers (a block: column-major on the host, relaid).  run(b, x): the driver.
template <class F>
int cx_krylov(mg_hierarchy* h, const double* b, double* x, long long n, long long maxIter, CxCols W, bool device_form, F&& run) {
  MG_TRY(W.ready(h, n, CX_ANY));
  if (!b || !x) return fail(MG_ERR_INVALID, "null %s", W.noun());
  if (maxIter < 0) return fail(MG_ERR_INVALID, "maxIter < 0");
  if (device_form) MG_TRY(cxv_aligned({b, x}));
  (void)hipSetDevice(h->device);
  MG_TRY(W.ensure(h));
  CxState& S = *h->cx;
  if (S.single && !S.K.set) MG_TRY(cx_widen_K(h));   // the Krylov product is never single
  if (device_form) return run(ccx(b), mcx(x));
  DevBuf<double>&sb = W.stage_b(S), &sx = W.stage_x(S);
  if (W.nr == 0 && sx.n != 2 * (size_t)n) MG_TRY(sx.alloc(2 * (size_t)n));   // (the vector iterate's staging buffer: sized on first use)
  MG_TRY(W.upload(h, b, S.Bstage_t, cxp(sb), n));
  MG_TRY(W.upload(h, x, S.Bstage_t, cxp(sx), n));
  MG_TRY(run(cxc(sb), cxp(sx)));
  MG_TRY(W.download(h, cxc(sx), S.Bstage_t, x, n));
  HIP_TRY(spin_sync(h->play->stream));
  return MG_OK;
}

// G = X^H Y by the one-pass kernel on its own (mg_cblk_gram_dev_CFP64): partials in `work`, the k x k result in `out`
int cx_gram_alone(const cx_t* X, const cx_t* Y, long long n, long long k, cx_t* work, cx_t* out, hipStream_t s) {
  if (n < 1) return fail(MG_ERR_INVALID, "a complex Gram matrix needs n >= 1");
  if (k < 1) return fail(MG_ERR_INVALID, "a complex Gram matrix needs k >= 1");
  if (k > mgk::BLK_KMAX) return fail(MG_ERR_UNSUPPORTED, "complex blocks hold at most %d columns (k=%lld)", mgk::BLK_KMAX, k);
  MG_TRY(cxv_aligned({X, Y, work, out}));
  int lg = 0;
  while ((1 << lg) < k) ++lg;
  const long long tr = mgk::GRAM_TILE >> lg;
  const int nb = (int)std::min<long long>(CxBlkKry::GRAM_WGS, (n + tr - 1) / tr);
  hipLaunchKernelGGL(mgk::cx_blk_gram_onepass, dim3(nb), dim3(mgk::BLK), 0, s, X, Y, n, (int)k, lg, work);
  hipLaunchKernelGGL(mgk::cx_blk_gram_final_wave, dim3((int)(k * k)), dim3(64), 0, s, work, nb, (int)k, out);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}

// One cycle on device vectors or blocks (row-major [n][nrhs]), ComplexF64, 16-byte aligned, enqueued on the handle's stream without a
// synchronisation.  A CF32 handle runs the reference's mixed closure on the whole vector or block, from zero: bl .= b; recursiveCycle
// from z = 0; z2 .= z (SolveFuncs.jl:52-58).
int cx_cycle_dev(mg_hierarchy* h, const double* b_dev, double* x_dev, long long n, long long x_is_zero, CxCols W, const char* who) {
  MG_TRY(W.ready(h, n, CX_ANY));
  if (!b_dev || !x_dev) return fail(MG_ERR_INVALID, "null %s", W.noun());
  if (x_is_zero != 0 && x_is_zero != 1) return fail(MG_ERR_INVALID, "x_is_zero must be 0 or 1 for device %ss", W.noun());
  MG_TRY(cxv_aligned({b_dev, x_dev}));
  if (h->cx->single && !x_is_zero)
    return fail(MG_ERR_UNSUPPORTED, "%s on a CF32 handle starts from zero (x_is_zero = 1): the mixed closure always zeroes z", who);
  (void)hipSetDevice(h->device);
  MG_TRY(W.ensure(h));
  CxLevel& L0 = h->cx->lev[0];
  const long long len = (long long)W.len(n);
  const size_t bytes = sizeof(cx_t) * (size_t)len;
  int xi = 0;
  if (h->cx->single) {
    MG_TRY(cx_narrow(h, ccx(b_dev), cxp<cf_t>(W.b(L0)), len));
    MG_TRY(cx_cycle<cf_t>(h, 0, cxc<cf_t>(W.b(L0)), xi, true, h->cycle, W.nr));
    return cx_widen(h, cxc<cf_t>(W.x(L0, xi)), mcx(x_dev), len);
  }
  if (!x_is_zero) HIP_TRY(hipMemcpyAsync(W.x(L0, xi).p, x_dev, bytes, hipMemcpyDeviceToDevice, h->play->stream));
  MG_TRY(cx_cycle<cx_t>(h, 0, ccx(b_dev), xi, x_is_zero == 1, h->cycle, W.nr));
  HIP_TRY(hipMemcpyAsync(x_dev, W.x(L0, xi).p, bytes, hipMemcpyDeviceToDevice, h->play->stream));
  return MG_OK;
}

}  // namespace

// =================================================================================================
// C ABI: the ComplexF64 Krylov drivers, their system operator, the device-pointer cycle and the passes on their own
// =================================================================================================
extern "C" {

int mg_set_krylov_operator_CFP64_INT64(mg_hierarchy* h, long long n, const long long* colptr, const long long* rowval,
                                       const double* nzval) {
  UploadFence upload_fence;
  MG_TRY(cx_level_ok(h, 1, CX_ANY));
  CxState& S = *h->cx;
  (void)hipSetDevice(h->device);
  HIP_TRY(spin_sync(h->play->stream));
  S.K_auto = false;   // (a widened As[1] is replaced or dropped below)
  if (!colptr) {   // back to As[1]; also on a handle that is not finalized (the way out when mg_finalize refuses a stale operator)
    S.K.release();
    return MG_OK;
  }
  if (!S.finalized) return fail(MG_ERR_STATE, "hierarchy not finalized: call mg_finalize before setting a Krylov operator");
  if (n != S.lev[0].n) return fail(MG_ERR_INVALID, "Krylov operator of order %lld on a fine level of %lld rows", n, S.lev[0].n);
  return cx_upload(&S.K, h->opt, n, n, colptr, rowval, nzval, true);   // (a failed upload leaves the handle on As[1])
}

int mg_cycle_dev_CFP64(mg_hierarchy* h, const double* b_dev, double* x_dev, long long n, long long x_is_zero) {
  return cx_cycle_dev(h, b_dev, x_dev, n, x_is_zero, CxCols::vec(), __func__);
}
int mg_block_cycle_dev_CFP64(mg_hierarchy* h, const double* b_dev, double* x_dev, long long n, long long nrhs, long long x_is_zero) {
  return cx_cycle_dev(h, b_dev, x_dev, n, x_is_zero, CxCols::blk(nrhs), __func__);
}

// blockBiCGSTB on the whole block: b, x column-major n x nrhs on the host (mg_block_bicgstab_CFP64) or row-major [n][nrhs] device
// blocks (_dev); x goes in and out; resvec holds up to 2*maxIter + 1 entries: max_j ||r_j|| / ||b_j|| at the start, after every
// half step and after every full step.
int mg_block_bicgstab_CFP64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs, double tol, long long maxIter,
                            long long* iters, long long* flag, double* resvec, long long* nres) {
  return cx_krylov(h, b, x, n, maxIter, CxCols::blk(nrhs), false, [&](const cx_t* B, cx_t* X) {
    return cx_block_bicgstab_dev(h, B, X, (int)nrhs, tol, maxIter, iters, flag, resvec, nres);
  });
}
int mg_block_bicgstab_dev_CFP64(mg_hierarchy* h, const double* b_dev, double* x_dev, long long n, long long nrhs, double tol,
                                long long maxIter, long long* iters, long long* flag, double* resvec, long long* nres) {
  return cx_krylov(h, b_dev, x_dev, n, maxIter, CxCols::blk(nrhs), true, [&](const cx_t* B, cx_t* X) {
    return cx_block_bicgstab_dev(h, B, X, (int)nrhs, tol, maxIter, iters, flag, resvec, nres);
  });
}
// blockFGMRES(inner) on the whole block, arguments as mg_block_fgmres[_dev]_FP64, layout as mg_block_bicgstab[_dev]_CFP64; resvec holds
// up to maxIter * inner entries, ||xi - H Y||_F / ||B||_F after every inner step; iters is the total number of inner steps.
int mg_block_fgmres_CFP64(mg_hierarchy* h, const double* b, double* x, long long n, long long nrhs, long long inner, double tol,
                          long long maxIter, long long* iters, long long* flag, double* resvec, long long* nres) {
  if (inner < 1 || inner > 64) return fail(MG_ERR_INVALID, "inner must be in [1,64]");
  return cx_krylov(h, b, x, n, maxIter, CxCols::blk(nrhs), false, [&](const cx_t* B, cx_t* X) {
    return cx_block_fgmres_dev(h, B, X, (int)nrhs, inner, tol, maxIter, iters, flag, resvec, nres);
  });
}
int mg_block_fgmres_dev_CFP64(mg_hierarchy* h, const double* b_dev, double* x_dev, long long n, long long nrhs, long long inner,
                              double tol, long long maxIter, long long* iters, long long* flag, double* resvec, long long* nres) {
  if (inner < 1 || inner > 64) return fail(MG_ERR_INVALID, "inner must be in [1,64]");
  return cx_krylov(h, b_dev, x_dev, n, maxIter, CxCols::blk(nrhs), true, [&](const cx_t* B, cx_t* X) {
    return cx_block_fgmres_dev(h, B, X, (int)nrhs, inner, tol, maxIter, iters, flag, resvec, nres);
  });
}

int mg_bicgstab_dev_CFP64(mg_hierarchy* h, const double* b_dev, double* x_dev, long long n, double tol, long long maxIter,
                          long long* iters, long long* flag, double* resvec, long long* nres) {
  return cx_krylov(h, b_dev, x_dev, n, maxIter, CxCols::vec(), true,
                   [&](const cx_t* bv, cx_t* xv) { return cx_bicgstab_dev(h, bv, xv, tol, maxIter, iters, flag, resvec, nres); });
}
int mg_bicgstab_CFP64(mg_hierarchy* h, const double* b, double* x, long long n, double tol, long long maxIter, long long* iters,
                      long long* flag, double* resvec, long long* nres) {
  return cx_krylov(h, b, x, n, maxIter, CxCols::vec(), false,
                   [&](const cx_t* bv, cx_t* xv) { return cx_bicgstab_dev(h, bv, xv, tol, maxIter, iters, flag, resvec, nres); });
}
int mg_fgmres_dev_CFP64(mg_hierarchy* h, const double* b_dev, double* x_dev, long long n, long long inner, double tol,
                        long long maxIter, long long* iters, long long* flag, double* resvec, long long* nres) {
  if (inner < 1 || inner > 64) return fail(MG_ERR_INVALID, "inner must be in [1,64]");
  return cx_krylov(h, b_dev, x_dev, n, maxIter, CxCols::vec(), true,
                   [&](const cx_t* bv, cx_t* xv) { return cx_fgmres_dev(h, bv, xv, inner, tol, maxIter, iters, flag, resvec, nres); });
}
int mg_fgmres_CFP64(mg_hierarchy* h, const double* b, double* x, long long n, long long inner, double tol, long long maxIter,
                    long long* iters, long long* flag, double* resvec, long long* nres) {
  if (inner < 1 || inner > 64) return fail(MG_ERR_INVALID, "inner must be in [1,64]");
  return cx_krylov(h, b, x, n, maxIter, CxCols::vec(), false,
                   [&](const cx_t* bv, cx_t* xv) { return cx_fgmres_dev(h, bv, xv, inner, tol, maxIter, iters, flag, resvec, nres); });
}

// ---- the passes on their own (tests, callers with Krylov loops of their own): asynchronous on `stream`; workspace_dev >= 8192
//      doubles, out_dev receives the pass's sums over the n elements; complex scalars are (re, im) pairs on the host ----
#define CXV_STREAM reinterpret_cast<hipStream_t>(stream)
#define CXV_C(p) cx_t{(p)[0], (p)[1]}
int mg_cvec_dots_dev_CFP64(long long k, const double* const* xs_dev, const double* const* ys_dev, long long n, double* workspace_dev,
                           double* out_dev, void* stream) {
  return cxv_dots((int)std::min<long long>(std::max<long long>(k, 0), mgcv::MAXD + 1), xs_dev, ys_dev, n, workspace_dev, out_dev, CXV_STREAM);
}
int mg_cvec_scale_dev_CFP64(const double* a, const double* x, double* y, long long n, void* stream) {
  if (!a) return fail(MG_ERR_INVALID, "null scalar");
  return cxv_launch(mgcv::OpCScale{CXV_C(a), ccx(x), mcx(y)}, n, {x, y}, nullptr, 0, nullptr, CXV_STREAM);
}
int mg_cvec_bicg_p_dev_CFP64(const double* beta, const double* omega, const double* r, const double* v, double* p, long long n,
                             void* stream) {
  if (!beta || !omega) return fail(MG_ERR_INVALID, "null scalar");
  return cxv_launch(mgcv::OpCBicgP{CXV_C(beta), CXV_C(omega), ccx(r), ccx(v), mcx(p)}, n, {r, v, p}, nullptr, 0, nullptr, CXV_STREAM);
}
int mg_cvec_bicg_s_dev_CFP64(const double* alpha, const double* v, double* r, long long n, double* workspace_dev, double* out_dev,
                             void* stream) {
  if (!alpha) return fail(MG_ERR_INVALID, "null scalar");
  return cxv_launch(mgcv::OpCBicgS{CXV_C(alpha), ccx(v), mcx(r)}, n, {v, r}, workspace_dev, 1, out_dev, CXV_STREAM);
}
int mg_cvec_bicg_ts_dev_CFP64(const double* t, const double* s, long long n, double* workspace_dev, double* out_dev, void* stream) {
  return cxv_launch(mgcv::OpCBicgTS{ccx(t), ccx(s)}, n, {t, s}, workspace_dev, 3, out_dev, CXV_STREAM);
}
int mg_cvec_bicg_xr_dev_CFP64(const double* alpha, const double* omega, const double* phat, const double* shat, const double* t,
                              const double* rtld, double* x, double* r, long long n, double* workspace_dev, double* out_dev,
                              void* stream) {
  if (!alpha || !omega) return fail(MG_ERR_INVALID, "null scalar");
  return cxv_launch(mgcv::OpCBicgXR{CXV_C(alpha), CXV_C(omega), ccx(phat), ccx(shat), ccx(t), ccx(rtld), mcx(x), mcx(r)}, n,
                    {phat, shat, t, rtld, x, r}, workspace_dev, 3, out_dev, CXV_STREAM);
}
int mg_cvec_gs_update_dev_CFP64(long long m, const double* h_host, const double* const* vs_dev, double* w, long long n,
                                double* workspace_dev, double* out_dev, void* stream) {
  if (m < 1 || m > 64 || !h_host || !vs_dev || !w || n < 1 || !workspace_dev)
    return fail(MG_ERR_INVALID, "gs_update: 1 to 64 vectors, non-null arguments");
  return cxv_gs_update((int)m, h_host, vs_dev, w, n, workspace_dev, out_dev, CXV_STREAM);
}
// G = X^H Y of two row-major blocks [n][k] by the one-pass Gram kernel of block FGMRES; workspace_dev: 2048 * k * k doubles,
// out_dev: the k x k complex result, row-major
int mg_cblk_gram_dev_CFP64(const double* x_dev, const double* y_dev, long long n, long long k, double* workspace_dev, double* out_dev,
                           void* stream) {
  return cx_gram_alone(ccx(x_dev), ccx(y_dev), n, k, mcx(workspace_dev), mcx(out_dev), CXV_STREAM);
}
#undef CXV_C
#undef CXV_STREAM

}  // extern "C"
