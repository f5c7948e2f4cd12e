// mg_krylov.inc - part of libmgvcycle.so's single translation unit (included by mgvcycle.hip in this order; not compiled on its own).
// Device-resident Krylov drivers with the cycle as preconditioner: PCG, BiCGSTAB, FGMRES and their block variants.
// FGMRES(m) is written once: fgmres_loop below runs the single-GPU / ghost-layer space (FgmresCore, here), the halo form's (mg_dist_krylov.inc)
// and the ComplexF64 one (mg_complex_krylov.inc).  The host algebra - KrylovReport (the outputs and the epilogue of every driver),
// HessenbergLsq, SmallMat / sm_*, pinv_sym - is mg_krylov_host.hpp.
namespace {
// Where the handle is one rank's extended boxes (ghost-layer form, mg_ghost.inc; round 6) the drivers below run SHARDED: every vector
// is n_ext long with its owned rows valid, a dot or norm is the sum over the owned rows of all ranks (box dot + one all-reduce; scalars
// due at the same point of an iteration share one), a product with A is taken behind ONE exchange of its input's ghost layers, the
// preconditioner is the sharded cycle as it is.  jInv enters the package through these drivers (SolveFuncs.jl:74-133, MGWrapper.jl:67-78).
struct KrylovSpace {
  mg_hierarchy* h;
  Level& L;
  const long long n;
  const bool ghs;
  explicit KrylovSpace(mg_hierarchy* h_) : h(h_), L(h_->lev[0]), n(h_->lev[0].n), ghs(gh_global_scalars(h_)) {}
  int dot(const double* x, const double* y, double* out) {
    if (!ghs) return dot_sync(h, x, y, n, out);
    return gh_dots_own(h, 1, &x, &y, out);
  }
  int dot2(const double* x1, const double* y1, const double* x2, const double* y2, double* o1, double* o2) {
    if (!ghs) {
      MG_TRY(dot_sync(h, x1, y1, n, o1));
      return dot_sync(h, x2, y2, n, o2);
    }
    const double* xs[2] = {x1, x2};
    const double* ys[2] = {y1, y2};
    double o[2];
    MG_TRY(gh_dots_own(h, 2, xs, ys, o));
    *o1 = o[0];
    *o2 = o[1];
    return MG_OK;
  }
  int norm(const double* x, double* out) {
    if (!ghs) return norm_sync(h, x, n, out);
    MG_TRY(gh_dots_own(h, 1, &x, &x, out));
    *out = std::sqrt(*out);
    return MG_OK;
  }
  int apply(double* x, double* y) {            // y = A x
    if (ghs) MG_TRY(gh_refresh(h, x));
    return k_spmv(h, 0, MG_K_SPMV, L.A, 1.0, x, 0.0, y);
  }
  int residual(const double* b, double* x, double* r) {   // r = b - A x
    if (ghs) MG_TRY(gh_refresh(h, x));
    return k_residual(h, 0, L.A, b, x, r);
  }
  int done() { return ghs ? gh_check_depths(h) : (int)MG_OK; }
};

// ---- the drivers' own launches by name: pcg_dev and FgmresCore::arnoldi below and the entry points mg_kry_*_dev_FP64 (mg_cabi.inc) run
// these, so the grid, the partial buffer and the stream of a pass are chosen in one place ------------------------------------------------
// x += alpha p ; r -= alpha Ap
int cg_update(mg_hierarchy* h, double alpha, const double* p, const double* Ap, double* x, double* r, long long n) {
  hipLaunchKernelGGL(mgk::cg_update_xr, dim3(grid_for(n)), dim3(mgk::BLK), 0, h->play->stream, alpha, p, Ap, x, r, n);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
// the same with *rn = ||r|| of the new r out of the pass; synchronises the stream
int cg_update_norm(mg_hierarchy* h, double alpha, const double* p, const double* Ap, double* x, double* r, long long n, double* rn) {
  const int nb = (int)std::min<long long>(grid_for(n), (long long)h->play->partial.n);
  hipLaunchKernelGGL(mgk::cg_update_xr_norm, dim3(nb), dim3(mgk::BLK), 0, h->play->stream, alpha, p, Ap, x, r, n, h->play->partial.p);
  launch_sum_final(h, h->play->partial.p, nb);
  HIP_TRY(hipGetLastError());
  return scalar_sync(h, rn);
}
// p = z + beta p
int cg_direction(mg_hierarchy* h, double beta, const double* z, double* p, long long n) {
  hipLaunchKernelGGL(mgk::cg_update_p, dim3(grid_for(n)), dim3(mgk::BLK), 0, h->play->stream, beta, z, p, n);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
// The chain dot -> update -> dot of modified Gram-Schmidt, every scalar in HBM.  mgs_blocks: the workgroups of each of its reductions;
// mgs_dot: *out = x.y ; mgs_update: w -= (*hk) v, then *out = w.u (u == nullptr: w.w) from the same pass.  hk, out: device; no synchronisation.
int mgs_blocks(mg_hierarchy* h, long long n) {
  return (int)std::min<long long>(h->nred_blocks, std::max<long long>(1, (n / 2 + mgk::BLK - 1) / mgk::BLK));
}
void mgs_dot(mg_hierarchy* h, const double* x, const double* y, long long n, double* out) {
  const int nb = mgs_blocks(h, n);
  hipLaunchKernelGGL(mgk::dot_partial, dim3(nb), dim3(mgk::BLK), 0, h->play->stream, x, y, n, h->play->partial.p);
  hipLaunchKernelGGL(mgk::sum_final, dim3(1), dim3(mgk::BLK), 0, h->play->stream, h->play->partial.p, nb, out);
}
void mgs_update(mg_hierarchy* h, const double* hk, const double* v, double* w, const double* u, long long n, double* out) {
  const int nb = mgs_blocks(h, n);
  hipLaunchKernelGGL(mgk::mgs_step, dim3(nb), dim3(mgk::BLK), 0, h->play->stream, hk, v, w, u, n, h->play->partial.p);
  hipLaunchKernelGGL(mgk::sum_final, dim3(1), dim3(mgk::BLK), 0, h->play->stream, h->play->partial.p, nb, out);
}
// One inner step's orthogonalisation: V holds i + 2 vectors n apart, w = the last against V_0 .. V_i, then w /= ||w|| unless it vanished.
// The i + 2 scalars (h_0 .. h_i, ||w||^2) come back in ONE readback: h->h_kscal, valid on return (the stream is drained).  slots: the
// scalars the device column is sized for (the caller's m + 2 >= i + 2).
int mgs_chain(mg_hierarchy* h, double* V, long long n, int i, size_t slots) {
  if (h->kscal.n < slots) MG_TRY(h->kscal.alloc(slots));
  if (!h->h_kscal) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->h_kscal), sizeof(double) * 66));
  double* w = V + (size_t)(i + 1) * n;
  double* hd = h->kscal.p;
  mgs_dot(h, w, V, n, hd);
  for (int k = 0; k <= i; ++k)
    mgs_update(h, hd + k, V + (size_t)k * n, w, k < i ? V + (size_t)(k + 1) * n : (const double*)nullptr, n, hd + k + 1);
  hipLaunchKernelGGL(mgk::scale_rsqrt, dim3(grid_for(n)), dim3(mgk::BLK), 0, h->play->stream, hd + i + 1, w, n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h->h_kscal, hd, sizeof(double) * (size_t)(i + 2), hipMemcpyDeviceToHost, h->play->stream));
  HIP_TRY(spin_sync(h->play->stream));
  return MG_OK;
}

// Preconditioned CG with one multigrid cycle (x = 0 on entry) as M: solveCG_MG (SolveFuncs.jl:104-116) ->
// KrylovMethods.cg (v0.6.0, un-vendored: Manifest.toml:35-41), restated from its published algorithm:
//   r = b - A x0 ; z = M r ; p = z ; nr0 = ||b||
//   loop: Ap = A p ; gamma = r.z ; alpha = gamma / p.Ap ; (alpha == Inf || alpha < 0 -> flag -2)
//         x += alpha p ; r -= alpha Ap ; resvec = ||r||/nr0 ; (<= tol -> flag 0)
//         z = M r ; beta = z.r / gamma ; p = z + beta p
int pcg_dev(mg_hierarchy* h, const double* b, double* x, double tol, long long maxIter, long long* iters,
            long long* flag_out, double* resvec) {
  Level& L = h->lev[0];
  const long long n = L.n;
  if (h->play->nrhs != 1) return fail(MG_ERR_UNSUPPORTED, "mg_pcg: block right-hand sides (KrylovMethods.blockCG) are not on the device path yet");
  if (h->kr.n != (size_t)n) {
    MG_TRY(h->kr.alloc((size_t)n));
    MG_TRY(h->kz.alloc((size_t)n));
    MG_TRY(h->kp.alloc((size_t)n));
    MG_TRY(h->kAp.alloc((size_t)n));
  }
  double* r = h->kr.p;
  double* z = h->kz.p;
  double* p = h->kp.p;
  double* Ap = h->kAp.p;
  KrylovSpace K(h);
  double nr0 = 0.0;
  MG_TRY(K.norm(b, &nr0));
  long long it = 0, flag = -1;
  KrylovReport rep(iters, flag_out, resvec, nullptr);
  if (nr0 == 0.0) {  // cg returns zeros, flag -9
    MG_TRY(k_fill(h, x, n, 0.0));
    HIP_TRY(spin_sync(h->play->stream));
    return rep.finish(0, -9);
  }
  MG_TRY(K.residual(b, x, r));                                         // r = b - A(x)
  MG_TRY(cycle_dev(h, r, z, true));                                    // z = M(r), x = 0 on entry
  HIP_TRY(hipMemcpyAsync(p, z, sizeof(double) * n, hipMemcpyDeviceToDevice, h->play->stream));
  // Three passes of the textbook loop are folded into their neighbours (same values, fewer sweeps over the vectors and one
  // host synchronisation less per iteration): gamma = r'z of iteration k+1 IS z'r of iteration k (computed once); p'Ap comes
  // out of the product kernel where the marching kernel serves A (partials of p[row]*Ap[row]); ||r||^2 out of the update.
  double gamma = 0.0;
  MG_TRY(K.dot(r, z, &gamma));
  for (long long k = 1; k <= maxIter; ++k) {
    it = k;
    double pAp = 0.0, rn = 0.0;
    if (K.ghs) {                                                       // sharded: p's ghost layers travel, sums over the owned rows
      MG_TRY(K.apply(p, Ap));
      MG_TRY(K.dot(p, Ap, &pAp));
    } else {
      MG_TRY(k_spmv_dot(h, 0, L.A, p, Ap, &pAp));                      // Ap = A(p), p'Ap
    }
    const double alpha = gamma / pAp;
    if (std::isinf(alpha) || alpha < 0.0) { flag = -2; break; }
    if (K.ghs) {
      MG_TRY(cg_update(h, alpha, p, Ap, x, r, n));
      MG_TRY(K.norm(r, &rn));
    } else {
      MG_TRY(cg_update_norm(h, alpha, p, Ap, x, r, n, &rn));
    }
    rep.set(k - 1, rn / nr0);
    if (rn / nr0 <= tol) { flag = 0; break; }
    MG_TRY(cycle_dev(h, r, z, true));
    double zr = 0.0;
    MG_TRY(K.dot(z, r, &zr));
    const double beta = zr / gamma;
    gamma = zr;                                                        // = r'z at the top of the next iteration
    MG_TRY(cg_direction(h, beta, z, p, n));
  }
  HIP_TRY(spin_sync(h->play->stream));
  rep.finish(it, flag);
  return K.done();
}

// Preconditioned BiCGSTAB with the multigrid cycle as M1 (M2 = identity): solveBiCGSTAB_MG (SolveFuncs.jl:87-101)
// -> KrylovMethods.bicgstb (v0.6.0, un-vendored).  Restated from the published algorithm (van der Vorst 1992 as in
// Barrett et al., "Templates", which KrylovMethods follows): resvec[0] = ||r0||/||b||, then two entries per
// iteration (||s||/||b|| after the first half step, ||r||/||b|| after the second); flags: 0 converged,
// -1 maxIter, -2 breakdown (rho == 0 or omega == 0), -3 converged on the half step, -9 b == 0.
int bicgstab_dev(mg_hierarchy* h, const double* b, double* x, double tol, long long maxIter, long long* iters,
                 long long* flag_out, double* resvec, long long* nres) {
  Level& L = h->lev[0];
  const long long n = L.n;
  if (h->play->nrhs != 1) return fail(MG_ERR_UNSUPPORTED, "mg_bicgstab: block right-hand sides (blockBiCGSTB) are not on the device path yet");
  if (h->kr.n != (size_t)n) {
    MG_TRY(h->kr.alloc((size_t)n));
    MG_TRY(h->kz.alloc((size_t)n));
    MG_TRY(h->kp.alloc((size_t)n));
    MG_TRY(h->kAp.alloc((size_t)n));
  }
  if (h->kw.n != (size_t)n * 4) MG_TRY(h->kw.alloc((size_t)n * 4));
  double* r = h->kr.p;       // residual, then s
  double* phat = h->kz.p;    // M p / M s
  double* p = h->kp.p;
  double* v = h->kAp.p;
  double* rtld = h->kw.p;
  double* t = h->kw.p + n;
  double* shat = h->kw.p + 2 * n;
  KrylovSpace K(h);
  double bn = 0.0, err = 0.0;
  MG_TRY(K.norm(b, &bn));
  long long it = 0, flag = -1;
  KrylovReport rep(iters, flag_out, resvec, nres);
  if (bn == 0.0) {
    MG_TRY(k_fill(h, x, n, 0.0));
    HIP_TRY(spin_sync(h->play->stream));
    return rep.finish(0, -9);
  }
  MG_TRY(K.residual(b, x, r));
  MG_TRY(K.norm(r, &err));
  err /= bn;
  rep.record(err);
  if (err < tol) return rep.finish(0, 0);
  HIP_TRY(hipMemcpyAsync(rtld, r, sizeof(double) * n, hipMemcpyDeviceToDevice, h->play->stream));
  double omega = 1.0, alpha = 0.0, rho1 = 0.0;
  for (long long k = 1; k <= maxIter; ++k) {
    it = k;
    double rho = 0.0;
    MG_TRY(K.dot(rtld, r, &rho));
    if (rho == 0.0) { flag = -2; break; }
    if (k > 1) {
      const double beta = (rho / rho1) * (alpha / omega);
      MG_TRY(k_axpby(h, -omega, v, 1.0, p, n));      // p = p - omega v
      MG_TRY(k_axpby(h, 1.0, r, beta, p, n));        // p = r + beta p
    } else {
      HIP_TRY(hipMemcpyAsync(p, r, sizeof(double) * n, hipMemcpyDeviceToDevice, h->play->stream));
    }
    MG_TRY(cycle_dev(h, p, phat, true));              // p_hat = M1(p)
    MG_TRY(K.apply(phat, v));
    double rv = 0.0;
    MG_TRY(K.dot(rtld, v, &rv));
    alpha = rho / rv;
    MG_TRY(k_axpby(h, -alpha, v, 1.0, r, n));         // s = r - alpha v (in r)
    double sn = 0.0;
    MG_TRY(K.norm(r, &sn));
    rep.record(sn / bn);
    if (sn / bn < tol) {                              // converged on the half step
      MG_TRY(k_axpby(h, alpha, phat, 1.0, x, n));
      flag = -3;
      break;
    }
    MG_TRY(cycle_dev(h, r, shat, true));              // s_hat = M1(s)
    MG_TRY(K.apply(shat, t));
    double ts = 0.0, tt = 0.0;
    MG_TRY(K.dot2(t, r, t, t, &ts, &tt));             // (sharded: the two scalars of omega in one all-reduce)
    omega = ts / tt;
    MG_TRY(k_axpby(h, alpha, phat, 1.0, x, n));
    MG_TRY(k_axpby(h, omega, shat, 1.0, x, n));       // x += alpha p_hat + omega s_hat
    MG_TRY(k_axpby(h, -omega, t, 1.0, r, n));         // r = s - omega t
    MG_TRY(K.norm(r, &err));
    err /= bn;
    rep.record(err);
    if (err <= tol) { flag = 0; break; }
    if (omega == 0.0) { flag = -2; break; }
    rho1 = rho;
  }
  HIP_TRY(spin_sync(h->play->stream));
  rep.finish(it, flag);
  return K.done();
}

// Flexible restarted GMRES with a (right) preconditioner: solveGMRES_MG (SolveFuncs.jl:119-133) -> KrylovMethods.fgmres (v0.6.0,
// un-vendored), restated from the published algorithm (Saad's FGMRES(m): Gram-Schmidt Arnoldi, Givens rotations, residual estimate
// |s_{i+1}|/||b|| after every inner step).  maxIter counts restarts, m is the Krylov dimension; resvec gets one entry per inner step;
// flag 0 converged, -1 not, -9 b = 0.  This is the ONE outer loop of every form - single GPU and ghost-layer (FgmresCore below), halo
// (DistFgmres, mg_dist_krylov.inc), ComplexF64 (CxFgmres, mg_complex_krylov.inc).  The small least squares is HessenbergLsq<S>
// (mg_krylov_host.hpp); everything that touches a vector is the space's:
//   norm_b(&bn)          ||b||                                     zero_x()             x = 0 (the b = 0 exit)
//   residual(&rn)        r = b - A x and ||r||                     start_basis(rn)      V_0 = r / ||r||
//   arnoldi(i, G)        z = M v_i, w = A z, orthogonalise against v_0 .. v_i, normalise into v_{i+1}; G.h(0..i, i) and G.hsub(i) = ||w||
//   update_x(used, y)    x += Z y                                  sync(), done()       drain the stream; what the exit owes
template <class S, class Space>
int fgmres_loop(Space& sp, int m, double tol, long long maxIter, KrylovReport& rep) {
  double bn = 0.0, rn = 0.0;
  MG_TRY(sp.norm_b(&bn));
  if (bn == 0.0) {
    MG_TRY(sp.zero_x());
    MG_TRY(sp.sync());
    return rep.finish(0, -9);
  }
  MG_TRY(sp.residual(&rn));
  double err = rn / bn;
  if (err < tol) return rep.finish(0, 0);
  HessenbergLsq<S> G(m);
  long long flag = -1, total = 0;
  for (long long it = 1; it <= maxIter && flag != 0; ++it) {
    MG_TRY(sp.start_basis(rn));                                            // V[:,1] = r/||r||
    G.begin(rn);
    int used = 0;
    for (int i = 0; i < m; ++i) {
      MG_TRY(sp.arnoldi(i, G));
      err = G.close_column(i) / bn;
      rep.record(err);
      ++total;
      used = i + 1;
      if (err <= tol) { flag = 0; break; }
    }
    MG_TRY(sp.update_x(used, G.solve(used).data()));                       // x += Z y
    if (flag == 0) break;
    MG_TRY(sp.residual(&rn));
    err = rn / bn;
    if (err <= tol) { flag = 0; break; }
  }
  MG_TRY(sp.sync());
  rep.finish(total, flag);
  return sp.done();
}

// The space of fgmres_core: level `lv` (0-based) of a single-GPU handle, or the fine level of one rank's extended boxes.
// precond 0: one multigrid cycle from level 0 (solveGMRES_MG, lv must be 0); precond 1: z = dprec .* v (the Jacobi-preconditioned
// coarsest solve, MGcycle.jl:152-168).
struct FgmresCore {
  mg_hierarchy* h;
  const int lv, precond, m;
  const double* dprec;
  const double* b;
  double* x;
  Level& L;
  const long long n;
  KrylovSpace K;
  const bool ghs;                             // (sharded: the fine level of one rank's extended boxes)
  double *V, *Z, *r;                          // m+1 basis vectors, m preconditioned vectors, residual / w
  FgmresCore(mg_hierarchy* h_, int lv_, int precond_, int m_, const double* dprec_, const double* b_, double* x_, double* work)
      : h(h_), lv(lv_), precond(precond_), m(m_), dprec(dprec_), b(b_), x(x_), L(h_->lev[(size_t)lv_]), n(L.n), K(h_), ghs(K.ghs && lv_ == 0),
        V(work), Z(work + (size_t)(m_ + 1) * n), r(Z + (size_t)m_ * n) {}
  int knorm(const double* v, double* out) { return ghs ? K.norm(v, out) : norm_sync(h, v, n, out); }
  int norm_b(double* out) { return knorm(b, out); }
  int zero_x() { return k_fill(h, x, n, 0.0); }
  int sync() {
    HIP_TRY(spin_sync(h->play->stream));
    return MG_OK;
  }
  int done() { return ghs ? K.done() : (int)MG_OK; }
  int residual(double* rn) {
    if (ghs) MG_TRY(gh_refresh(h, x));
    MG_TRY(k_residual(h, lv, L.A, b, x, r));
    return knorm(r, rn);
  }
  int start_basis(double rn) { return k_axpby(h, 1.0 / rn, r, 0.0, V, n); }
  int arnoldi(int i, HessenbergLsq<double>& G) {
    double* vi = V + (size_t)i * n;
    double* zi = Z + (size_t)i * n;
    double* w = V + (size_t)(i + 1) * n;
    if (precond == 0) MG_TRY(cycle_dev(h, vi, zi, true));               // z = M(V[:,i])
    else MG_TRY(k_dscale(h, lv, dprec, vi, zi, n));
    if (ghs) MG_TRY(gh_refresh(h, zi));                                 // (sharded: z's ghost layers from their owners)
    MG_TRY(k_spmv(h, lv, MG_K_SPMV, L.A, 1.0, zi, 0.0, w));             // w = A z
    // modified Gram-Schmidt with the chain dot -> update -> dot on the device: h_k = w.V_k stays in HBM, the update
    // w -= h_k V_k reads it there and produces the partials of the next dot (or of ||w||^2) in the same pass; the i+2
    // scalars come back in ONE readback per inner step (round 2: one host synchronisation instead of i+2)
    if (h->opt.no_mgs_chain || ghs) {   // (A/B: one dot, one host synchronisation and one update per basis vector; sharded: every
                                        // dot is a sum over the owned rows of all ranks - one all-reduce per basis vector, as MGS orders them)
      for (int k = 0; k <= i; ++k) {
        double hk = 0.0;
        if (ghs) MG_TRY(K.dot(w, V + (size_t)k * n, &hk));
        else MG_TRY(dot_sync(h, w, V + (size_t)k * n, n, &hk));
        G.h(k, i) = hk;
        MG_TRY(k_axpby(h, -hk, V + (size_t)k * n, 1.0, w, n));
      }
      double wn = 0.0;
      MG_TRY(knorm(w, &wn));
      G.hsub(i) = wn;
      if (wn != 0.0) MG_TRY(k_axpby(h, 1.0 / wn, w, 0.0, w, n));
    } else {
      MG_TRY(mgs_chain(h, V, n, i, (size_t)m + 2));
      for (int k = 0; k <= i; ++k) G.h(k, i) = h->h_kscal[k];
      G.hsub(i) = std::sqrt(h->h_kscal[i + 1]);
    }
    return MG_OK;
  }
  int update_x(int used, const double* y) {
    for (int i = 0; i < used; ++i) MG_TRY(k_axpby(h, y[i], Z + (size_t)i * n, 1.0, x, n));
    return MG_OK;
  }
};

int fgmres_core(mg_hierarchy* h, int lv, int precond, const double* dprec, DevBuf<double>& work, const double* b,
                double* x, long long inner, double tol, long long maxIter, long long* iters, long long* flag_out,
                double* resvec, long long* nres) {
  const long long n = h->lev[(size_t)lv].n;
  if (h->play->nrhs != 1) return fail(MG_ERR_UNSUPPORTED, "fgmres: block right-hand sides (blockFGMRES) are not on the device path yet");
  if (inner < 1 || inner > 64) return fail(MG_ERR_INVALID, "inner must be in [1,64]");
  const int m = (int)inner;
  if (work.n != (size_t)n * (size_t)(2 * m + 2)) MG_TRY(work.alloc((size_t)n * (size_t)(2 * m + 2)));
  FgmresCore sp(h, lv, precond, m, dprec, b, x, work.p);
  KrylovReport rep(iters, flag_out, resvec, nres);
  return fgmres_loop<double>(sp, m, tol, maxIter, rep);
}

int fgmres_dev(mg_hierarchy* h, const double* b, double* x, long long inner, double tol, long long maxIter,
               long long* iters, long long* flag_out, double* resvec, long long* nres) {
  return fgmres_core(h, 0, 0, nullptr, h->kw, b, x, inner, tol, maxIter, iters, flag_out, resvec, nres);
}

// ---- block Krylov drivers (SolveFuncs.jl:95,113,130 -> KrylovMethods.blockBiCGSTB / blockCG / blockFGMRES) -----------
// The package is not vendored; the published algorithms (DESIGN.md section 4: O'Leary's block CG, El Guennouni-Jbilou-
// Sadok block BiCGSTAB, block flexible GMRES) are implemented here with every n x k block resident in HBM (row-major [n][k], k <= 16): products with A
// are SpMM launches, the preconditioner is one cycle on the whole block, k x k Gram matrices come back through one
// 8*k*k-byte readback each, and the small dense algebra (pseudo-inverse, LU solve, triangular factor, block least
// squares) runs on the host: SmallMat, sm_* and pinv_sym of mg_krylov_host.hpp.
// G = X'Y (k x k) to the host; synchronises the stream
int blk_gram(mg_hierarchy* h, const double* X, const double* Y, long long n, int k, SmallMat& G) {
  if (gh_global_scalars(h) && n == h->lev[0].n) {   // sharded: the Gram matrix over the owned rows of all ranks (one all-reduce of k*k doubles)
    G = SmallMat(k, k);
    return gh_gram_own(h, X, Y, k, G.a.data(), h->blk_partial);
  }
  const int nb = (int)std::min<long long>(256, std::max<long long>(1, (n + mgk::BLK - 1) / mgk::BLK));
  if (h->blk_partial.n < (size_t)nb * k * k + (size_t)k * k) MG_TRY(h->blk_partial.alloc((size_t)nb * k * k + (size_t)k * k));
  if (!h->h_blk) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->h_blk), sizeof(double) * mgk::BLK_KMAX * mgk::BLK_KMAX));
  double* out = h->blk_partial.p + (size_t)nb * k * k;
  hipLaunchKernelGGL(mgk::blk_gram_partial, dim3(nb, k), dim3(mgk::BLK), 0, h->play->stream, X, Y, n, k, h->blk_partial.p);
  hipLaunchKernelGGL(mgk::blk_gram_final, dim3(1), dim3(mgk::BLK), 0, h->play->stream, h->blk_partial.p, nb, k, out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h->h_blk, out, sizeof(double) * k * k, hipMemcpyDeviceToHost, h->play->stream));
  HIP_TRY(spin_sync(h->play->stream));
  G = SmallMat(k, k);
  std::memcpy(G.a.data(), h->h_blk, sizeof(double) * k * k);
  return MG_OK;
}
// out = s*add + in*C   (add may be null; out may alias in or add)
int blk_comb(mg_hierarchy* h, double* out, const double* add, double s, const double* in, const SmallMat& Cm, long long n, int k) {
  if (h->blk_c.n < (size_t)mgk::BLK_KMAX * mgk::BLK_KMAX * 8) MG_TRY(h->blk_c.alloc((size_t)mgk::BLK_KMAX * mgk::BLK_KMAX * 8));
  // a ring of 8 coefficient slots (pinned host + device): copies are asynchronous and earlier launches may still read
  // theirs; the stream is drained once per lap of the ring
  constexpr size_t SLOT = (size_t)mgk::BLK_KMAX * mgk::BLK_KMAX;
  if (!h->h_blk_c) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->h_blk_c), sizeof(double) * SLOT * 8));
  const unsigned si = h->blk_c_next++ % 8;
  if (si == 0 && h->blk_c_next > 1) HIP_TRY(spin_sync(h->play->stream));
  double* slot = h->blk_c.p + si * SLOT;
  std::memcpy(h->h_blk_c + si * SLOT, Cm.a.data(), sizeof(double) * k * k);
  HIP_TRY(hipMemcpyAsync(slot, h->h_blk_c + si * SLOT, sizeof(double) * k * k, hipMemcpyHostToDevice, h->play->stream));
  hipLaunchKernelGGL(mgk::blk_comb, dim3(grid_for(n)), dim3(mgk::BLK), 0, h->play->stream, out, add, s, in, slot, n, k);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
int blk_colnorms(mg_hierarchy* h, const double* X, long long n, int k, std::vector<double>& out) {
  SmallMat G;
  MG_TRY(blk_gram(h, X, X, n, k, G));
  out.assign((size_t)k, 0.0);
  for (int j = 0; j < k; ++j) out[(size_t)j] = std::sqrt(std::max(0.0, G(j, j)));
  return MG_OK;
}
int blk_work(mg_hierarchy* h, size_t nblocks, long long n, int k, double** base) {
  const size_t need = nblocks * (size_t)n * (size_t)k;
  if (h->kw.n < need) MG_TRY(h->kw.alloc(need));
  *base = h->kw.p;
  return MG_OK;
}

// Sharded (ghost-layer form, round 6): the blocks are [n_ext][k] with their owned rows valid - a product with A follows ONE exchange of
// the block's ghost layers, the preconditioner is the block's columns through the sharded cycle, Gram matrices are sums over owned rows.
int blk_apply(mg_hierarchy* h, int lv, double* P, double* Q) {
  if (lv == 0 && gh_global_scalars(h)) MG_TRY(gh_exchange_block(h, P, (int)h->play->nrhs));
  return k_spmv(h, lv, MG_K_SPMV, h->lev[(size_t)lv].A, 1.0, P, 0.0, Q);
}
int blk_residual(mg_hierarchy* h, int lv, const double* B, double* X, double* R) {
  if (lv == 0 && gh_global_scalars(h)) MG_TRY(gh_exchange_block(h, X, (int)h->play->nrhs));
  return k_residual(h, lv, h->lev[(size_t)lv].A, B, X, R);
}
int blk_cycle(mg_hierarchy* h, const double* R, double* Z) {
  if (h->ghost) return cycle_dev_columns(h, R, Z, true);
  return cycle_dev(h, R, Z, true);
}

// blockCG (O'Leary 1980): Alpha = pinv(P'Q) P'R ; X += P Alpha ; R -= Q Alpha ; Beta = -pinv(P'Q) Q'Z ; P = Z + P Beta
int block_pcg_dev(mg_hierarchy* h, const double* B, double* X, double tol, long long maxIter, long long* iters,
                  long long* flag_out, double* resmat) {
  Level& L = h->lev[0];
  const long long n = L.n;
  const int k = (int)h->play->nrhs;
  if (k > mgk::BLK_KMAX) return fail(MG_ERR_UNSUPPORTED, "block Krylov drivers hold at most %d right-hand sides", mgk::BLK_KMAX);
  const size_t len = (size_t)n * k;
  double* w = nullptr;
  MG_TRY(blk_work(h, 4, n, k, &w));
  double *R = w, *Z = w + len, *P = w + 2 * len, *Q = w + 3 * len;
  std::vector<double> nb, rn;
  MG_TRY(blk_colnorms(h, B, n, k, nb));
  long long it = 0, flag = -1;
  KrylovReport rep(iters, flag_out, nullptr, nullptr);   // (resmat is iterations x k, written where it is computed)
  bool any = false;
  for (double v : nb) any = any || v > 0.0;
  if (!any) {
    MG_TRY(k_fill(h, X, (long long)len, 0.0));
    HIP_TRY(spin_sync(h->play->stream));
    return rep.finish(0, -9);
  }
  for (double& v : nb) if (!(v > 0.0)) v = 1.0;
  MG_TRY(blk_residual(h, 0, B, X, R));                         // R = B - A X
  MG_TRY(blk_cycle(h, R, Z));                               // Z = M(R)
  HIP_TRY(hipMemcpyAsync(P, Z, sizeof(double) * len, hipMemcpyDeviceToDevice, h->play->stream));
  for (long long iter = 1; iter <= maxIter; ++iter) {
    it = iter;
    MG_TRY(blk_apply(h, 0, P, Q));         // Q = A P
    SmallMat PTQ, PTR, QTZ;
    MG_TRY(blk_gram(h, P, Q, n, k, PTQ));
    MG_TRY(blk_gram(h, P, R, n, k, PTR));
    std::vector<double> Hs((size_t)k * k), Pinv;
    for (int i = 0; i < k; ++i)
      for (int j = 0; j < k; ++j) Hs[(size_t)i * k + j] = 0.5 * (PTQ(i, j) + PTQ(j, i));
    pinv_sym(Hs, k, Pinv);
    SmallMat Pi(k, k);
    Pi.a = Pinv;
    const SmallMat Alpha = sm_mul(Pi, PTR);
    MG_TRY(blk_comb(h, X, X, 1.0, P, Alpha, n, k));               // X += P Alpha
    SmallMat negAlpha = Alpha;
    for (double& v : negAlpha.a) v = -v;
    MG_TRY(blk_comb(h, R, R, 1.0, Q, negAlpha, n, k));            // R -= Q Alpha
    MG_TRY(blk_colnorms(h, R, n, k, rn));
    double worst = 0.0;
    for (int j = 0; j < k; ++j) {
      const double rel = rn[(size_t)j] / nb[(size_t)j];
      if (resmat) resmat[(size_t)(iter - 1) * k + j] = rel;
      worst = std::max(worst, rel);
    }
    if (worst <= tol) { flag = 0; break; }
    MG_TRY(blk_cycle(h, R, Z));
    MG_TRY(blk_gram(h, Q, Z, n, k, QTZ));
    SmallMat Beta = sm_mul(Pi, QTZ);
    for (double& v : Beta.a) v = -v;
    MG_TRY(blk_comb(h, P, Z, 1.0, P, Beta, n, k));                // P = Z + P Beta
  }
  HIP_TRY(spin_sync(h->play->stream));
  return rep.finish(it, flag);
}

// blockBiCGSTB (El Guennouni, Jbilou, Sadok 2003), right-preconditioned by the cycle
int block_bicgstab_dev(mg_hierarchy* h, const double* B, double* X, double tol, long long maxIter, long long* iters,
                       long long* flag_out, double* resvec, long long* nres) {
  Level& L = h->lev[0];
  const long long n = L.n;
  const int k = (int)h->play->nrhs;
  if (k > mgk::BLK_KMAX) return fail(MG_ERR_UNSUPPORTED, "block Krylov drivers hold at most %d right-hand sides", mgk::BLK_KMAX);
  const size_t len = (size_t)n * k;
  double* w = nullptr;
  MG_TRY(blk_work(h, 7, n, k, &w));
  double *R = w, *R0 = w + len, *P = w + 2 * len, *Ph = w + 3 * len, *V = w + 4 * len, *Sh = w + 5 * len, *T = w + 6 * len;
  std::vector<double> nb, rn;
  MG_TRY(blk_colnorms(h, B, n, k, nb));
  long long it = 0, flag = -1;
  KrylovReport rep(iters, flag_out, resvec, nres);
  bool any = false;
  for (double v : nb) any = any || v > 0.0;
  if (!any) {
    MG_TRY(k_fill(h, X, (long long)len, 0.0));
    HIP_TRY(spin_sync(h->play->stream));
    return rep.finish(0, -9);
  }
  for (double& v : nb) if (!(v > 0.0)) v = 1.0;
  auto worst_rel = [&](const double* blk, double* out) -> int {
    MG_TRY(blk_colnorms(h, blk, n, k, rn));
    double wv = 0.0;
    for (int j = 0; j < k; ++j) wv = std::max(wv, rn[(size_t)j] / nb[(size_t)j]);
    *out = wv;
    return MG_OK;
  };
  MG_TRY(blk_residual(h, 0, B, X, R));
  double err = 0.0;
  MG_TRY(worst_rel(R, &err));
  rep.record(err);
  if (err < tol) return rep.finish(0, 0);
  HIP_TRY(hipMemcpyAsync(R0, R, sizeof(double) * len, hipMemcpyDeviceToDevice, h->play->stream));
  HIP_TRY(hipMemcpyAsync(P, R, sizeof(double) * len, hipMemcpyDeviceToDevice, h->play->stream));
  const SmallMat I1 = sm_scaled_identity(k, 1.0);
  for (long long iter = 1; iter <= maxIter; ++iter) {
    it = iter;
    MG_TRY(blk_cycle(h, P, Ph));                            // Phat = M(P)
    MG_TRY(blk_apply(h, 0, Ph, V));        // V = A Phat
    SmallMat RtV, RtR, alpha;
    MG_TRY(blk_gram(h, R0, V, n, k, RtV));
    MG_TRY(blk_gram(h, R0, R, n, k, RtR));
    if (!sm_solve(RtV, RtR, alpha)) { flag = -2; break; }
    SmallMat nalpha = alpha;
    for (double& v : nalpha.a) v = -v;
    MG_TRY(blk_comb(h, R, R, 1.0, V, nalpha, n, k));              // S = R - V alpha   (in R)
    double sn = 0.0;
    MG_TRY(worst_rel(R, &sn));
    rep.record(sn);
    if (sn < tol) {
      MG_TRY(blk_comb(h, X, X, 1.0, Ph, alpha, n, k));
      flag = -3;
      break;
    }
    MG_TRY(blk_cycle(h, R, Sh));                            // Shat = M(S)
    MG_TRY(blk_apply(h, 0, Sh, T));        // T = A Shat
    SmallMat TS, TT;
    MG_TRY(blk_gram(h, T, R, n, k, TS));
    MG_TRY(blk_gram(h, T, T, n, k, TT));
    double ts = 0.0, tt = 0.0;
    for (int j = 0; j < k; ++j) { ts += TS(j, j); tt += TT(j, j); }
    if (tt == 0.0) { flag = -2; break; }
    const double omega = ts / tt;
    MG_TRY(blk_comb(h, X, X, 1.0, Ph, alpha, n, k));              // X += Phat alpha + omega Shat
    MG_TRY(blk_comb(h, X, X, 1.0, Sh, sm_scaled_identity(k, omega), n, k));
    MG_TRY(blk_comb(h, R, R, 1.0, T, sm_scaled_identity(k, -omega), n, k));   // R = S - omega T
    MG_TRY(worst_rel(R, &err));
    rep.record(err);
    if (err <= tol) { flag = 0; break; }
    if (omega == 0.0) { flag = -2; break; }
    SmallMat RtT, beta;
    MG_TRY(blk_gram(h, R0, T, n, k, RtT));
    if (!sm_solve(RtV, RtT, beta)) { flag = -2; break; }
    for (double& v : beta.a) v = -v;
    MG_TRY(blk_comb(h, P, P, 1.0, V, sm_scaled_identity(k, -omega), n, k));   // P - omega V
    MG_TRY(blk_comb(h, P, R, 1.0, P, beta, n, k));                // P = R + (P - omega V) beta
  }
  HIP_TRY(spin_sync(h->play->stream));
  return rep.finish(it, flag);
}

// W -> orthonormal block (in place) by Cholesky QR applied twice; Rf with W_in = Q Rf
int blk_cholqr(mg_hierarchy* h, double* W, long long n, int k, SmallMat& Rf) {
  SmallMat G;
  MG_TRY(blk_gram(h, W, W, n, k, G));
  const SmallMat R1 = sm_chol_semidefinite(G);
  MG_TRY(blk_comb(h, W, nullptr, 0.0, W, sm_tri_pinv(R1), n, k));
  MG_TRY(blk_gram(h, W, W, n, k, G));
  const SmallMat R2 = sm_chol_semidefinite(G);
  MG_TRY(blk_comb(h, W, nullptr, 0.0, W, sm_tri_pinv(R2), n, k));
  Rf = sm_mul(R2, R1);
  return MG_OK;
}

// blockFGMRES: block flexible GMRES(inner), block modified Gram-Schmidt, exact block least squares per inner step
// lv: the level whose A is solved; precond 0: Z = one cycle from x = 0 (level 0 only), 1: Z = dprec .* V (the Jacobi
// preconditioner of the coarsest-level GMRES branch, MGcycle.jl:157-159); work: own work space (nullptr: the block drivers')
int block_fgmres_core(mg_hierarchy* h, int lv, int precond, const double* dprec, DevBuf<double>* work, const double* B,
                      double* X, long long inner, double tol, long long maxIter, long long* iters, long long* flag_out,
                      double* resvec, long long* nres) {
  Level& L = h->lev[(size_t)lv];
  const long long n = L.n;
  const int k = (int)h->play->nrhs;
  if (k > mgk::BLK_KMAX) return fail(MG_ERR_UNSUPPORTED, "block Krylov drivers hold at most %d right-hand sides", mgk::BLK_KMAX);
  if (inner < 1 || inner > 64) return fail(MG_ERR_INVALID, "inner must be in [1,64]");
  if (precond == 0 && lv != 0) return fail(MG_ERR_INVALID, "the cycle preconditions the fine level only");
  const int m = (int)inner;
  const size_t len = (size_t)n * k;
  double* w = nullptr;
  if (work) {
    const size_t need = (size_t)(2 * m + 2) * len;
    if (work->n < need) MG_TRY(work->alloc(need));
    w = work->p;
  } else {
    MG_TRY(blk_work(h, (size_t)(2 * m + 2), n, k, &w));
  }
  double* Vb = w;                              // m+1 blocks
  double* Zb = w + (size_t)(m + 1) * len;      // m blocks
  double* R = Zb + (size_t)m * len;            // residual / W
  long long flag = -1, total = 0;
  KrylovReport rep(iters, flag_out, resvec, nres);
  auto fro = [&](const double* blk, double* out) -> int {
    std::vector<double> cn;
    MG_TRY(blk_colnorms(h, blk, n, k, cn));
    double s2 = 0.0;
    for (double v : cn) s2 += v * v;
    *out = std::sqrt(s2);
    return MG_OK;
  };
  double bn = 0.0, rn = 0.0;
  MG_TRY(fro(B, &bn));
  if (bn == 0.0) {
    MG_TRY(k_fill(h, X, (long long)len, 0.0));
    HIP_TRY(spin_sync(h->play->stream));
    return rep.finish(0, -9);
  }
  MG_TRY(blk_residual(h, lv, B, X, R));
  MG_TRY(fro(R, &rn));
  if (rn / bn < tol) return rep.finish(0, 0);
  for (long long it = 1; it <= maxIter && flag != 0; ++it) {
    SmallMat H((m + 1) * k, m * k), xi((m + 1) * k, k), Rf, Y;
    HIP_TRY(hipMemcpyAsync(Vb, R, sizeof(double) * len, hipMemcpyDeviceToDevice, h->play->stream));
    MG_TRY(blk_cholqr(h, Vb, n, k, Rf));
    for (int i = 0; i < k; ++i)
      for (int j = 0; j < k; ++j) xi(i, j) = Rf(i, j);
    int used = 0;
    for (int j = 0; j < m; ++j) {
      double* Vj = Vb + (size_t)j * len;
      double* Zj = Zb + (size_t)j * len;
      double* W = Vb + (size_t)(j + 1) * len;
      if (precond == 0) MG_TRY(blk_cycle(h, Vj, Zj));        // Z_j = M(V_j)
      else MG_TRY(k_dscale(h, lv, dprec, Vj, Zj, n));
      MG_TRY(blk_apply(h, lv, Zj, W));      // W = A Z_j
      for (int i = 0; i <= j; ++i) {                               // block modified Gram-Schmidt
        SmallMat Hij;
        MG_TRY(blk_gram(h, Vb + (size_t)i * len, W, n, k, Hij));
        for (int a = 0; a < k; ++a)
          for (int b = 0; b < k; ++b) H(i * k + a, j * k + b) = Hij(a, b);
        for (double& v : Hij.a) v = -v;
        MG_TRY(blk_comb(h, W, W, 1.0, Vb + (size_t)i * len, Hij, n, k));
      }
      SmallMat Hn;
      MG_TRY(blk_cholqr(h, W, n, k, Hn));
      for (int a = 0; a < k; ++a)
        for (int b = 0; b < k; ++b) H((j + 1) * k + a, j * k + b) = Hn(a, b);
      SmallMat Hb((j + 2) * k, (j + 1) * k), xb((j + 2) * k, k);
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
      SmallMat Yj(k, k);
      for (int a = 0; a < k; ++a)
        for (int b = 0; b < k; ++b) Yj(a, b) = Y(j * k + a, b);
      MG_TRY(blk_comb(h, X, X, 1.0, Zb + (size_t)j * len, Yj, n, k));
    }
    if (flag == 0) break;
    MG_TRY(blk_residual(h, lv, B, X, R));
    MG_TRY(fro(R, &rn));
    if (rn / bn <= tol) { flag = 0; break; }
  }
  HIP_TRY(spin_sync(h->play->stream));
  return rep.finish(total, flag);
}
int block_fgmres_dev(mg_hierarchy* h, const double* B, double* X, long long inner, double tol, long long maxIter,
                     long long* iters, long long* flag_out, double* resvec, long long* nres) {
  return block_fgmres_core(h, 0, 0, nullptr, nullptr, B, X, inner, tol, maxIter, iters, flag_out, resvec, nres);
}

}  // namespace
