// mg_schedule.inc - part of libmgvcycle.so's single translation unit (included by mgvcycle.hip in this order; not compiled on its own).
// FGMRES relaxation (Jac-GMRES smoother, K-cycle; its least squares is RelaxLsq of mg_krylov_host.hpp), the level schedule (cycle_level, HIP graphs of the coarse sub-cycle), the solve loop.
namespace {
// ---- FGMRES_relaxation (FGMRES.jl:48-126) --------------------------------------------------------------
// The small least squares (pinv_sym, RelaxLsq) is host algebra: mg_krylov_host.hpp.
int k_axpby(mg_hierarchy* h, double a, const double* x, double b, double* y, long long n) {
  hipLaunchKernelGGL(mgk::axpby_kernel, dim3(grid_for(n)), dim3(mgk::BLK), 0, h->play->stream, a, x, b, y, n);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}

int dot_sync(mg_hierarchy* h, const double* x, const double* y, long long len, double* out);

// x0 += Z*t where t minimises ||r0 - A Z t|| over the `inner` directions z_1 = M r0, z_j = M (A z_{j-1}).
// prec(v, z) must write z = M v (length n*nrhs).  x0_is_zero: x0 is overwritten with the correction
// (K-cycle: xc = 0 on entry, MGcycle.jl:63-64, and x0 doubles as scratch of the inner cycles).
template <class Prec>
int fgmres_relax(mg_hierarchy* h, int lv, const double* r0, double* x0, long long inner, Prec prec,
                 double TOL, double* Zb, double* AZb, bool x0_is_zero) {
  Level& L = h->lev[(size_t)lv];
  const long long len = L.n * h->play->nrhs;
  if (inner <= 0) {
    if (x0_is_zero) MG_TRY(k_fill(h, x0, len, 0.0));
    return MG_OK;  // w = Z*t with no columns: x0 unchanged (FGMRES.jl:119-121)
  }
  const int k = (int)inner;
  // Ghost-layer form (a sharded level of one rank's extended boxes; round 6): norms and dots are sums over the owned rows of all ranks,
  // z's ghost layers travel in front of the product (one exchange per direction), the results are valid on the owned rows.
  const bool ghs = gh_sharded_sums(h, lv);
  if (ghs && h->play->nrhs != 1) return fail(MG_ERR_UNSUPPORTED, "ghost-layer form: the FGMRES relaxation runs on single vectors");
  auto gdot = [&](const double* x, const double* y, double* out) { return ghs ? gh_dots_own(h, 1, &x, &y, out, lv) : dot_sync(h, x, y, len, out); };
  double rnorm0 = 0.0;
  if (ghs) {
    MG_TRY(gdot(r0, r0, &rnorm0));
    rnorm0 = std::sqrt(rnorm0);
  } else {
    MG_TRY(norm_sync(h, r0, len, &rnorm0));
  }
  RelaxLsq Q(k);
  int used = 0;
  for (int j = 0; j < k; ++j) {
    double* z = Zb + (size_t)j * len;
    double* w = AZb + (size_t)j * len;
    MG_TRY(prec(j == 0 ? r0 : AZb + (size_t)(j - 1) * len, z));          // z = prec(r0) / prec(w)   (l.83-87)
    if (ghs) MG_TRY(gh_refresh(h, z, lv));
    MG_TRY(k_spmv(h, lv, MG_K_SPMV, L.A, 1.0, z, 0.0, w));                // w = A z                  (l.91)
    if (ghs) gh_set(h, lv, w, gh_dec(h, lv, GH_FULL));
    used = j + 1;
    for (int i = 0; i <= j; ++i) {                                       // t = AZ' * w              (l.95)
      double d = 0.0;
      MG_TRY(gdot(AZb + (size_t)i * len, w, &d));
      Q.set(i, j, d);
    }
    MG_TRY(gdot(w, r0, &Q.xi[(size_t)j]));                               // xi[j] = dot(w, r0)       (l.97)
    const double rn = Q.step(rnorm0);                                    // t = pinv(H)*xi, ||r0 - AZ t||  (l.102-104)
    if (rn < TOL) break;                                                          // l.114-117
  }
  for (int j = 0; j < used; ++j)                                         // x0 += Z*t                (l.121-123)
    MG_TRY(k_axpby(h, Q.t()[(size_t)j], Zb + (size_t)j * len, (j == 0 && x0_is_zero) ? 0.0 : 1.0, x0, len));
  if (ghs) gh_set(h, lv, x0, 0);      // (what is claimed of the result: its owned rows)
  return MG_OK;
}

// relaxation type 2: numit Vanka iterations of x in place on level l, from the operator the level already holds
int vanka_relax(mg_hierarchy* h, int l, const double* b, double* x, long long numit) {
  Level& L = h->lev[(size_t)l];
  if (!L.vanka) return fail(MG_ERR_STATE, "level %d has no Vanka blocks (mg_set_vanka_FP64)", l + 1);
  return vanka_run(L.vanka, L.A.rowptr.p, L.A.colidx.p, L.A.val.p, b, x, numit, L.vanka_type, h->play->stream);
}

// ---- the cycle ------------------------------------------------------------------------------------
// Returns in *result the buffer (xa or xb) that holds the level's x after the cycle.
// l is 0-based.  xa holds the incoming x when !x_zero; xb is the Jacobi ping-pong partner.
// r_valid: L.r already holds b - A*x for the incoming x (solveMG computed it for its stopping test,
// SolveFuncs.jl:26-30, and recursiveCycle would recompute the same values, MGcycle.jl:26-31).
// x1_ready (with r_valid): xb already holds xa + d.*r, the first pre-smoothing update (written by the residual kernel
// of the previous solve step, k_residual_sumsq's xnext).
int cycle_sub(mg_hierarchy* h, int l, const double* b, double* xa, double* xb, bool x_zero, char ctype, double** result,
              bool x1_given = false);
// x1_given (with x_zero): xa already holds d.*b, the first update from x = 0 (written by the restriction that produced b).
// defer_post (solve loop, fine level): leave the LAST post-smoothing sweep to the caller, who fuses it with the residual
// of the stopping test (k_smooth_residual); *defer_post says whether that happened (result = x before that sweep).
// pre_done (solve loop, fine level): the caller's four-stage pass already ran this level's pre-smoothing and residual -
// xa holds the smoothed x, L.r = b - A x: the cycle starts at the restriction.
int cycle_level(mg_hierarchy* h, int l, const double* b, double* xa, double* xb, bool x_zero,
                char ctype, double** result, bool r_valid = false, bool x1_ready = false, bool* defer_post = nullptr,
                bool x1_given = false, bool pre_done = false) {
  const int nl = (int)h->nlevels;
  if (l == nl - 1) {  // solveCoarsest (MGcycle.jl:13-18,67-69,177): x = LU \ b
    MG_TRY(k_coarse(h, l, b, xa, x_zero));
    *result = xa;
    return MG_OK;
  }
  Level& L = h->lev[l];
  Level& C = h->lev[l + 1];
  Play::Vecs& VC = h->play->lev[(size_t)l + 1];   // the coarse level's vectors and this level's residual, of the lane being played
  double* const Lr = h->play->res(l);
  const long long len = L.n * h->play->nrhs;
  double* cur = xa;
  double* alt = xb;
  const double gmresTol = 1e-5;  // MGcycle.jl:5
  auto diag_prec = [&](const double* v, double* z) { return k_dscale(h, l, L.d.p, v, z, L.n); };  // MM (l.36-38)
  // relax() always performs at least one update: `for i=1:numit-1 ... end; x .+= d.*r` (MGcycle.jl:127-134)
  long long npre = std::max<long long>(1, L.npre);
  const long long npost = std::max<long long>(1, L.npost);
  bool from_zero = false;
  // Ghost-layer form of a sharded level (mg_ghost.inc; every call below is a no-op on an ordinary level): dep = layers of ghost
  // nodes a vector is valid on, need = exchange the ghost layers first if fewer than that many are, setd = what an operation left.
  const bool gh = gh_level(h, l) != nullptr;
  const bool gh_any = h->ghost && h->ghost->finalized && l < h->ghost->a;   // (also a world of one going through RCCL)
  auto dep = [&](const double* v) { return gh_depth(h, l, v); };
  auto dec = [&](int d) { return gh_dec(h, l, d); };
  auto setd = [&](const double* v, int d) { if (gh) gh_set(h, l, v, d); };
  auto need = [&](const double* v, int want) { return gh ? gh_need(h, l, v, want) : (int)MG_OK; };
  // pre-smoothing (MGcycle.jl:26-31,54).  x == 0: r = b, so the first sweep is x = d.*b.
  if (pre_done) {
    npre = 0;
  } else if (h->relax_type == 2) {  // Vanka (MGcycle.jl:51-52): npre in-place iterations, none for a count of 0
    if (x_zero) MG_TRY(k_fill(h, cur, len, 0.0));
    MG_TRY(vanka_relax(h, l, b, cur, L.npre));
    npre = 0;
  } else if (h->relax_type == 1) {  // Jac-GMRES (MGcycle.jl:48-50): FGMRES on the residual, preconditioned by D
    const double* r0 = b;
    MG_TRY(need(b, 0));
    MG_TRY(need(cur, 0));
    if (x_zero) {
      MG_TRY(k_fill(h, cur, len, 0.0));
      setd(cur, GH_FULL);
    } else {
      if (!r_valid) {
        MG_TRY(need(cur, 1));
        MG_TRY(need(Lr, 0));
        MG_TRY(k_residual(h, l, L.A, b, cur, Lr));
        setd(Lr, std::min(dec(dep(cur)), dep(b)));
      }
      r0 = Lr;
    }
    MG_TRY(fgmres_relax(h, l, r0, cur, L.npre, diag_prec, gmresTol, L.relaxZ.p, L.relaxAZ.p, false));
    npre = 0;
  } else if (x_zero) {
    // two sweeps from x = 0 on a level the two-stage pass serves: x1 = d.*b is formed inside that pass
    from_zero = !x1_given && npre == 2 && !h->opt.no_march2_zero && march2_ok(h, l, cur, alt, Lr, nullptr) && zero_form_static(L.A) &&
                gh_agree_zero(h, l) && gh_agree2(h, l);                  // (sharded: what every rank's kernels can do)
    MG_TRY(need(b, 0));
    if (!from_zero && !x1_given) {
      MG_TRY(need(cur, 0));
      MG_TRY(k_dscale(h, l, L.d.p, b, cur, L.n));
      setd(cur, dep(b));
    }
    --npre;
  } else if (r_valid) {
    if (!x1_ready) {
      MG_TRY(need(cur, 0));
      MG_TRY(need(Lr, 0));
      MG_TRY(need(alt, 0));
      MG_TRY(k_xpdr(h, l, cur, L.d.p, Lr, alt, L.n));
      setd(alt, std::min(dep(cur), dep(Lr)));
    }
    std::swap(cur, alt);
    --npre;
  }
  // one damped-Jacobi sweep src -> dst with the bookkeeping of the ghost-layer form
  auto sweep = [&](const double* src, double* dst) -> int {
    MG_TRY(need(src, 1));
    MG_TRY(need(b, 0));
    MG_TRY(need(dst, 0));
    MG_TRY(k_smooth(h, l, L.A, L.d.p, b, src, dst));
    setd(dst, std::min(dec(dep(src)), dep(b)));
    return MG_OK;
  };
  // the last pre-smoothing sweep and r = b - A x (MGcycle.jl:58-60) in one pass where the marching kernel allows
  const bool fuse_pre = npre >= 1 && march2_ok(h, l, cur, alt, Lr, nullptr) && gh_agree2(h, l);
  for (long long s = 0; s < npre - (fuse_pre ? 1 : 0); ++s) {
    MG_TRY(sweep(cur, alt));
    std::swap(cur, alt);
  }
  // r = b - A x ; bc = R r ; xc = 0 (MGcycle.jl:58-66)
  const bool small_rr = !pre_done && !fuse_pre && !gh_any && small_fuse_rr_ok(h, l);
  if (pre_done) {
    // (L.r is the four-stage pass's r')
  } else if (fuse_pre) {
    if (from_zero) MG_TRY(need(b, 2));
    else { MG_TRY(need(cur, 2)); MG_TRY(need(b, 1)); }
    MG_TRY(need(alt, 0));
    MG_TRY(need(Lr, 0));
    MG_TRY(k_smooth_residual(h, l, b, cur, alt, Lr, nullptr, false, from_zero));
    const int dt = std::min(dec(from_zero ? dep(b) : dep(cur)), dep(b));
    setd(alt, dt);
    setd(Lr, std::min(dec(dt), dep(b)));
    std::swap(cur, alt);
  } else if (small_rr) {
    // (a small level: the residual is formed inside the restriction's launch, in LDS - grid27_small_resid_restrict)
  } else {
    MG_TRY(need(cur, 1));
    MG_TRY(need(b, 0));
    MG_TRY(need(Lr, 0));
    MG_TRY(k_residual(h, l, L.A, b, cur, Lr));
    setd(Lr, std::min(dec(dep(cur)), dep(b)));
  }
  if (gh) {
    // x comes back at the prolongation, a whole coarse cycle away: if it will not carry the post-smoothing (and the caller's fused
    // pass behind a deferred last sweep: four stages + the layer its restriction reads), its ghost layers travel meanwhile
    const long long inside = std::max<long long>(1, L.npost) - ((defer_post && *defer_post) ? 1 : 0);
    MG_TRY(gh_prefetch(h, l, cur, (int)inside + ((defer_post && *defer_post) ? 5 : 0)));
    MG_TRY(need(Lr, 1));     // the restriction reads the residual one layer around the owned coarse nodes
  }
  // the restriction also writes the coarse level's first update x = d.*bc where its kernel can (no dscale launch there)
  // (not into a sharded or just all-reduced level: its bc is complete only behind the exchange)
  // (into a sharded level both vectors travel in the one exchange behind the restriction; not into the just all-reduced level)
  // (nor where the coarse level's first fused pass forms x1 itself - its from-zero form: one vector less to write, read and exchange)
  const bool give_x1 = (!gh_any || l + 1 < h->ghost->a) && h->relax_type == 0 && !(ctype == 'K') && l + 1 < nl - 1 && C.relax_set && restrict_can_scale(h, L.R) && gh_agree_scale(h, l) &&
                       !from_zero_static(h, l + 1);
  if (small_rr) MG_TRY(k_small_resid_restrict(h, l, b, cur, VC.b.p, give_x1 ? C.d.p : nullptr, give_x1 ? VC.x0.p : nullptr));
  else MG_TRY(k_spmv(h, l, MG_K_RESTRICT, L.R, 1.0, Lr, 0.0, VC.b.p, give_x1 ? C.d.p : nullptr, give_x1 ? VC.x0.p : nullptr));
  if (gh_any) {
    if (l + 1 < h->ghost->a) {   // the coarse right-hand side: valid where the residual reached, then every ghost layer at once
      if (gh_level(h, l + 1)) {
        const int dr = std::min(dep(Lr), gh_level(h, l)->gmin);
        gh_set(h, l + 1, VC.b.p, (dr - 1) / 2);
        if (give_x1) {   // bc and x1 = d.*bc in one exchange
          gh_set(h, l + 1, VC.x0.p, (dr - 1) / 2);
          MG_TRY(gh_touch(h, l + 1, VC.b.p));
          MG_TRY(gh_touch(h, l + 1, VC.x0.p));
          MG_TRY(gh_exchange_start(h, l + 1, VC.b.p, VC.x0.p));
          MG_TRY(gh_exchange_finish(h, l + 1));
        } else {
          MG_TRY(gh_need(h, l + 1, VC.b.p, GH_FULL));
        }
      }
    } else {
      MG_TRY(gh_allreduce_tail(h, VC.b.p, C.n));   // rows of the first replicated level: every rank contributed the nodes it owns
    }
  }
  double* xc = nullptr;
  if (ctype == 'K' && l + 1 < nl - 1) {
    // K-cycle (MGcycle.jl:72-76): 2 steps of FGMRES on A_{l+1} xc = bc, preconditioned by the K-cycle of level l+1
    auto kprec = [&](const double* v, double* z) {
      double* res = nullptr;
      MG_TRY(cycle_level(h, l + 1, v, VC.x0.p, VC.x1.p, true, 'K', &res));
      MG_TRY(gh_touch(h, l + 1, res));
      HIP_TRY(hipMemcpyAsync(z, res, sizeof(double) * C.n * h->play->nrhs, hipMemcpyDeviceToDevice, h->play->stream));
      if (gh_level(h, l + 1)) gh_set(h, l + 1, z, gh_depth(h, l + 1, res));
      return (int)MG_OK;
    };
    MG_TRY(fgmres_relax(h, l + 1, VC.b.p, VC.x0.p, 2, kprec, gmresTol, C.kZ.p, C.kAZ.p, true));
    xc = VC.x0.p;
  } else {
    MG_TRY(cycle_sub(h, l + 1, VC.b.p, VC.x0.p, VC.x1.p, true, ctype, &xc, give_x1));
  }
  if (l + 1 < nl - 1) {  // MGcycle.jl:78-85
    if (ctype == 'W') {
      double* other = (xc == VC.x0.p) ? VC.x1.p : VC.x0.p;
      MG_TRY(cycle_sub(h, l + 1, VC.b.p, xc, other, false, 'W', &xc));
    } else if (ctype == 'F') {
      double* other = (xc == VC.x0.p) ? VC.x1.p : VC.x0.p;
      MG_TRY(cycle_sub(h, l + 1, VC.b.p, xc, other, false, 'V', &xc));
    }
  }
  // x += P xc (MGcycle.jl:90) and post-smoothing (l.92-102)
  const long long post_done = 0;
  int gh_after_p = GH_FULL;   // what x + P xc is valid on
  if (gh) {
    // A fine node d layers outside the owned box interpolates from coarse nodes up to ceil((d + 1) / 2) layers outside theirs: a
    // correction valid on k >= 1 layers gives 2k - 1 (all of them: every layer - a level's box holds the parents of the finer box's
    // nodes).  Its ghost layers travel only where that falls short of what the post-smoothing (and the caller's fused pass behind a
    // deferred last sweep) consume.
    if (l + 1 < h->ghost->a && gh_level(h, l + 1)) {
      const long long want = std::max<long long>(1, L.npost) - ((defer_post && *defer_post) ? 1 : 0) + ((defer_post && *defer_post) ? 5 : 0);
      auto reach = [&]() { const int k = gh_depth(h, l + 1, xc); return k >= GH_FULL ? GH_FULL : 2 * k - 1; };
      if (reach() < std::min<long long>(want, gh_level(h, l)->gmin)) MG_TRY(gh_need(h, l + 1, xc, GH_FULL));
      else MG_TRY(gh_touch(h, l + 1, xc));
      gh_after_p = reach();
    }
    MG_TRY(need(cur, 0));
  }
  // (a small level: the corrected x is formed inside the first post-sweep's launch, in LDS - grid27_small_prolong_smooth)
  long long nlast = npost;
  if (defer_post && *defer_post && post_done < npost) --nlast;   // the caller runs the last sweep (fused with its residual)
  const bool small_ps = !gh_any && h->relax_type == 0 && nlast > post_done && cur != alt && small_fuse_ps_ok(h, l);
  long long swept = post_done;
  if (small_ps) {
    MG_TRY(k_small_prolong_smooth(h, l, xc, cur, b, alt));
    std::swap(cur, alt);
    ++swept;
  } else {
    MG_TRY(k_spmv(h, l, MG_K_PROLONG, L.P, 1.0, xc, 1.0, cur));
  }
  if (gh) setd(cur, std::min(dep(cur), gh_after_p));
  if (h->relax_type == 2) {   // MGcycle.jl:99-100
    MG_TRY(vanka_relax(h, l, b, cur, L.npost));
  } else if (h->relax_type == 1) {
    MG_TRY(need(cur, 1));
    MG_TRY(need(b, 0));
    MG_TRY(need(Lr, 0));
    MG_TRY(k_residual(h, l, L.A, b, cur, Lr));
    setd(Lr, std::min(dec(dep(cur)), dep(b)));
    MG_TRY(fgmres_relax(h, l, Lr, cur, L.npost, diag_prec, gmresTol, L.relaxZ.p, L.relaxAZ.p, false));
  } else {
    if (!(defer_post && *defer_post && post_done < npost) && defer_post) *defer_post = false;
    for (long long s = swept; s < nlast; ++s) {
      MG_TRY(sweep(cur, alt));
      std::swap(cur, alt);
    }
  }
  if (defer_post && h->relax_type != 0) *defer_post = false;
  *result = cur;
  return MG_OK;
}

// Setup entry points copy with blocking hipMemcpy on the NULL stream while every kernel runs on the handle's
// non-blocking stream, which does not order against it.  A blocking copy from pageable memory may return once the
// data sits in the runtime's staging buffer, the DMA still in flight (seen on MI355X: a solve launched right after
// an upload read zeros).  Every uploading entry point therefore ends with a device-wide fence.
struct UploadFence {
  ~UploadFence() { (void)hipDeviceSynchronize(); }
};

// sharded_ok: the entry point is one the ghost-layer form serves (mg_cycle_dev_FP64 / mg_solve_dev_FP64 and the device Krylov drivers,
// single-vector and block: exchanges inside, sums over the owned rows of all ranks).  Everything else on a handle that is one rank's
// extended boxes - host-pointer entry points, products whose sums would run over ghost rows - is refused rather than computed on the
// wrong rows.
int check_ready(mg_hierarchy* h, long long n, long long nrhs, bool sharded_ok = false) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  if (!h->finalized) return fail(MG_ERR_STATE, "hierarchy not finalized: call mg_finalize first");
  if (h->ghost && !sharded_ok)
    return fail(MG_ERR_UNSUPPORTED, "this handle is one rank's part of a sharded hierarchy (mg_ghost_attach): mg_cycle_dev_FP64, mg_solve_dev_FP64 and the device Krylov drivers (mg_pcg_dev / mg_bicgstab_dev / mg_fgmres_dev and their block forms) run on it");
  if (h->ghost && !h->ghost->finalized) return fail(MG_ERR_STATE, "mg_ghost_finalize was not called");
  if (n != h->lev[0].n) return fail(MG_ERR_INVALID, "n=%lld does not match the fine level (%lld rows)", n, h->lev[0].n);
  if (h->relax_type == 2 && (h->nrhs != 1 || h->cycle == 'K' || h->ghost))
    return fail(MG_ERR_UNSUPPORTED, "Vanka relaxation (type 2): one right-hand side, V / W / F cycles, unsharded handles");
  if (nrhs != h->nrhs)
    return fail(MG_ERR_INVALID, "nrhs=%lld but the scratch is sized for %lld: call mg_set_nrhs (adjustMemoryForNumRHS)", nrhs, h->nrhs);
  return MG_OK;
}

void graphs_clear(mg_hierarchy* h) {
  if (h->graphs.empty()) return;
  if (h->play->stream) (void)spin_sync(h->play->stream);   // a replay may still be running
  for (Play* p : h->lanes)   // (the column-wise block solve replays graphs on its own streams too)
    if (p->stream) (void)spin_sync(p->stream);
  for (auto& kv : h->graphs) {
    if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    if (kv.second.graph) (void)hipGraphDestroy(kv.second.graph);
  }
  h->graphs.clear();
}

// The levels below a few hundred thousand rows are launch-bound (8-14 us per kernel for microseconds of work): the
// whole sub-cycle from the first such level down - smoothers, transfers, coarsest solve, every launch with fixed
// arguments on hierarchy-owned buffers - is captured once into a HIP graph and replayed.  Not for cycles with host
// decisions inside (Jac-GMRES smoothing, K-cycles, GMRES coarsest solve), not with a Schwarz sweep as coarsest solve (its large
// members run on their appliers' own streams) and not while profiling (events per launch).
bool graph_ok(const mg_hierarchy* h, int l, char ctype) {
  if (h->opt.no_graph || h->prof || h->capturing || h->relax_type != 0 || ctype == 'K' || h->coarse_gmres || h->coarse_dd) return false;
  // a caller's stream (mg_set_stream) may be the legacy null stream, which cannot capture, or be part of a capture of
  // the caller's own: only the hierarchy's own stream is captured, unless the caller vouches for its stream (dist tail)
  if (!h->play->stream || (!h->play->owns_stream && !h->opt.dist_tail_graph)) return false;
  if (h->lev[(size_t)l].n * h->play->nrhs > h->opt.graph_max_rows) return false;
  if (h->ghost && l < h->ghost->a) return false;   // sharded levels: exchanges and an all-reduce inside (the replicated levels below replay as a graph)
  return (int)h->nlevels - l >= 2 || (h->coarse_lu && h->lu_multi);
}
int cycle_sub(mg_hierarchy* h, int l, const double* b, double* xa, double* xb, bool x_zero, char ctype, double** result,
              bool x1_given) {
  if (!graph_ok(h, l, ctype)) return cycle_level(h, l, b, xa, xb, x_zero, ctype, result, false, false, nullptr, x1_given);
  const mg_hierarchy::GraphKey key{l, x_zero, ctype, b, xa, xb, x1_given, h->play->nrhs};
  auto it = h->graphs.find(key);
  if (it == h->graphs.end()) {
    if (h->graphs.size() >= 64) graphs_clear(h);   // callers cycling through many buffers: start over
    mg_hierarchy::GraphEntry e;
    HIP_TRY(hipStreamBeginCapture(h->play->stream, hipStreamCaptureModeThreadLocal));
    h->capturing = true;
    const int rc = cycle_level(h, l, b, xa, xb, x_zero, ctype, &e.result, false, false, nullptr, x1_given);
    h->capturing = false;
    const hipError_t ce = hipStreamEndCapture(h->play->stream, &e.graph);
    if (rc != MG_OK || ce != hipSuccess) {
      if (e.graph) (void)hipGraphDestroy(e.graph);
      if (rc != MG_OK) return rc;
      HIP_TRY(ce);
    }
    HIP_TRY(hipGraphInstantiate(&e.exec, e.graph, nullptr, nullptr, 0));
    it = h->graphs.emplace(key, e).first;
  }
  HIP_TRY(hipGraphLaunch(it->second.exec, h->play->stream));
  ++h->graph_launches;
  *result = it->second.result;
  return MG_OK;
}

// one cycle on device buffers; result guaranteed to be in x on return (no sync)
int cycle_dev(mg_hierarchy* h, const double* b, double* x, bool x_zero) {
  double* res = nullptr;
  MG_TRY(gh_begin(h, &b, x, x_zero));   // (ghost-layer form: b with its ghost layers, bookkeeping reset)
  h->last_b = b;
  h->last_x = x;
  MG_TRY(cycle_sub(h, 0, b, x, h->play->lev[0].x1.p, x_zero, h->cycle, &res));
  if (res != x)
    HIP_TRY(hipMemcpyAsync(x, res, sizeof(double) * h->lev[0].n * h->play->nrhs, hipMemcpyDeviceToDevice, h->play->stream));
  return gh_check_depths(h);
}

// ---------------------------------------------------------------------------------------------------------------------------
// solveMG on device buffers (SolveFuncs.jl:3-39).  One step = one cycle + the residual and norm of the stopping test; three KINDS
// of step, one method each, chosen per step by what the fine level's kernels allow:
//   step_four_stage   the cycle left its last post-smoothing sweep undone (deferred) and the loop goes on by count: that sweep, the
//                     stopping test's residual + norm and the NEXT cycle's two pre-smoothing stages are one pass
//                     (csr_rowclass_march4_spmv); the norm is read one step later (pipelined stopping test);
//   step_last_sweep   deferred as well, but the last step by count or no four-stage form: last sweep + residual + norm (+ the next
//                     cycle's first update) in the two-stage pass;
//   step_residual     nothing deferred: residual + norm in one pass (every operator format).
// Buffers: `cur` holds the newest x (before a deferred sweep: the sweep's input), `alt` is free for the next result, `spare` the
// third buffer of the fused forms, `keep` the input of a four-stage step whose norm has not been read yet (untouched until then:
// if the test ends the loop at that step its iterate is re-created from `keep`).  The caller's x is one of the three.
// Ghost-layer form (mg_ghost.inc): the hierarchy is one rank's extended boxes - norms are sums over the owned rows of all ranks
// and every pass first asks for the ghost layers it consumes (need) and then records what its outputs are still valid on.
// ---------------------------------------------------------------------------------------------------------------------------
struct SolveLoop {
  mg_hierarchy* h;
  Level& L;
  double* const Lr;                        // the fine-level residual of the lane being played
  const double* b;
  double* x;
  const double tol;
  const long long maxIter;
  double* resvec;
  const long long len;
  bool ghs = false, gh0 = false;           // norms are sums over the ranks / the fine level exchanges ghost layers
  double res = 0.0, res0 = 0.0;
  long long it = 0;
  double *cur = nullptr, *alt = nullptr, *spare = nullptr, *keep = nullptr;
  bool fuse_post = false;                  // the cycle may leave its last post-smoothing sweep to the pass behind it
  bool x1_ready = false;                   // alt already holds the next cycle's first update x + d.*r
  bool pre_done = false;                   // cur is t' (the next cycle starts at its restriction), L.r its residual
  bool t_missing = false;                  // the iterate of the last step was not stored (dead while the loop goes on)
  bool stopped = false;                    // the loop ended at a pipelined step: cur was re-created from keep
  bool pending = false;                    // a four-stage step's norm has not been read yet
  int pending_slot = 0;

  SolveLoop(mg_hierarchy* h_, const double* b_, double* x_, double tol_, long long maxIter_, double* resvec_)
      : h(h_), L(h_->lev[0]), Lr(h_->play->res(0)), b(b_), x(x_), tol(tol_), maxIter(maxIter_), resvec(resvec_), len(h_->lev[0].n * h_->play->nrhs) {}

  int depth(const double* v) const { return gh_depth(h, 0, v); }
  int dec(int d) const { return gh_dec(h, 0, d); }
  int need(const double* v, int d) { return gh0 ? gh_need(h, 0, v, d) : MG_OK; }
  void valid_on(const double* v, int d) { if (gh0) gh_set(h, 0, v, d); }
  int norm_of(const double* v, double* out) { return ghs ? gh_norm_own(h, v, out) : norm_sync(h, v, len, out); }

  // SolveFuncs.jl:14-22: ||x||, then ||b|| or ||b - A x||; buffers and event slots of the loop.  *x_zero: x == 0 on entry
  int begin(bool* x_zero) {
    MG_TRY(gh_begin(h, &b, x, false));      // (ghost-layer form: b gets its ghost layers once, bookkeeping reset)
    ghs = gh_global_scalars(h);
    gh0 = gh_level(h, 0) != nullptr;
    h->last_b = b;
    h->last_x = x;
    double xn = 0.0;
    MG_TRY(norm_of(x, &xn));
    *x_zero = (xn == 0.0);
    if (*x_zero) {
      MG_TRY(norm_of(b, &res0));
    } else if (ghs) {
      MG_TRY(need(x, 1));
      MG_TRY(need(Lr, 0));
      MG_TRY(k_residual(h, 0, L.A, b, x, Lr));
      valid_on(Lr, std::min(dec(depth(x)), depth(b)));
      MG_TRY(gh_norm_own(h, Lr, &res0));
    } else {
      MG_TRY(k_residual_sumsq(h, 0, L.A, b, x, Lr));
      MG_TRY(scalar_sync(h, &res0));
    }
    res = res0;
    if (resvec) resvec[0] = res0;
    cur = x;
    alt = h->play->lev[0].x1.p;
    if (h->play->nrhs == 1 && !h->opt.no_march2 && !h->opt.no_fused_next && (L.A.rc_march2 || L.A.rc_march3) && std::max<long long>(1, L.npost) >= 1) {
      if (L.x2.n != (size_t)len) {
        MG_TRY(L.x2.alloc((size_t)len));
        HIP_TRY(hipMemsetAsync(L.x2.p, 0, L.x2.bytes(), h->play->stream));
      }
      spare = L.x2.p;
      fuse_post = march2_ok(h, 0, cur, alt, nullptr, spare) && march2_ok(h, 0, alt, spare, nullptr, cur) && march2_ok(h, 0, spare, cur, nullptr, alt) && gh_agree2(h, 0) && gh_agree_zero(h, 0);
    }
    if (!h->pipe_ev[0]) {
      HIP_TRY(hipEventCreateWithFlags(&h->pipe_ev[0], hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&h->pipe_ev[1], hipEventDisableTiming));
    }
    return MG_OK;
  }

  // one more entry of the residual history; true: the stopping test ends the loop here (SolveFuncs.jl:34-36)
  bool record(double r) {
    res = r;
    ++it;
    if (resvec) resvec[it] = res;
    return res / res0 < tol;
  }

  // read the pending four-stage step's norm (waits for its event)
  int read_pending(bool* stop) {
    if (!pending) return MG_OK;
    if (h->dsum.on && h->dsum.ev == h->pipe_ev[pending_slot]) MG_TRY(flush_deferred_sum(h));   // (nothing came behind the pass to take its sum along)
    hipError_t e;
    while ((e = hipEventQuery(h->pipe_ev[pending_slot])) == hipErrorNotReady) {
#if defined(__x86_64__)
      __builtin_ia32_pause();
#endif
    }
    HIP_TRY(e);
    MG_TRY(gh_host_reduce(h, h->h_scalar + 1 + pending_slot));   // (host-staged transport: the ranks' sums are added here)
    pending = false;
    if (record(std::sqrt(h->h_scalar[1 + pending_slot]))) *stop = true;
    return MG_OK;
  }

  // the loop ended at the step whose input is `keep`: whatever was enqueued behind it is dropped, its iterate re-created
  int finish_from_keep() {
    MG_TRY(flush_deferred_sum(h));   // (the dropped step's sum: nobody reads it, but nothing may stay pending)
    HIP_TRY(spin_sync(h->play->stream));
    double* dst = cur == keep ? alt : cur;
    MG_TRY(need(keep, 1));
    MG_TRY(need(dst, 0));
    MG_TRY(k_smooth(h, 0, L.A, L.d.p, b, keep, dst));
    valid_on(dst, std::min(dec(depth(keep)), depth(b)));
    cur = dst;
    stopped = true;
    return MG_OK;
  }

  // (ghost-layer form: the pass consumes FOUR ghost layers of x in one kernel - a fine level with fewer takes the two-stage steps)
  bool four_stage_serves(long long count, bool deferred) const {
    return deferred && count < maxIter && !h->opt.no_dead_t && march4_ok(h, 0, cur, alt, Lr) && (!gh0 || gh_level(h, 0)->gmin >= 4) && gh_agree4(h);
  }

  // cur (x before the last sweep) -> alt = t' (x after the next cycle's pre-smoothing), L.r = b - A t', ||r|| of THIS step into a
  // pinned slot behind an event.  The host reads the PREVIOUS step's norm only now, with this step already in the queue: the device
  // never waits for the host's round trip.  Speculative across the test (finish_from_keep).
  int step_four_stage(long long count, bool* stop) {
    const int slot = (int)(count & 1);
    MG_TRY(need(cur, 5));          // four products deep (+ the layer the restriction behind it reads, if the ghost layers reach that far)
    MG_TRY(need(b, 4));
    MG_TRY(need(alt, 0));
    MG_TRY(need(Lr, 0));
    bool sum_deferred = false;      // (single GPU: the partial sums are added up by one more workgroup of the next cycle's restriction)
    MG_TRY(k_four_stage(h, 0, b, cur, alt, Lr, h->h_scalar + 1 + slot, gh0 || h->ghost ? nullptr : h->pipe_ev[slot], gh0 || h->ghost ? nullptr : &sum_deferred));   // alt: neither cur nor keep
    if (gh0) {
      const int db = depth(b), dt = std::min(dec(depth(cur)), db), dr = std::min(dec(dt), db), dn = std::min(dt, dr);
      const int dp = std::min(dec(dn), db);
      valid_on(alt, dp);
      valid_on(Lr, std::min(dec(dp), db));
    }
    if (!sum_deferred) HIP_TRY(hipEventRecord(h->pipe_ev[slot], h->play->stream));
    MG_TRY(read_pending(stop));
    if (*stop) return finish_from_keep();
    double* freed = keep;                           // (verified: the previous step's input is free again)
    keep = cur;                                     // this step's input: untouched until its norm has been read
    cur = alt;                                      // t': the next cycle's x after pre-smoothing
    if (freed) alt = freed;
    else { alt = spare; spare = nullptr; }
    pending = true;
    pending_slot = slot;
    pre_done = true;
    x1_ready = false;
    if (h->opt.no_pipeline) {
      MG_TRY(read_pending(stop));
      if (*stop) return finish_from_keep();
    }
    return MG_OK;
  }

  // cur = x before the last sweep; alt <- the iterate; spare <- x + d.*r (unused if this was the last step).  The iterate itself is
  // DEAD while the loop goes on (the next cycle starts from x + d.*r and recomputes its own residual): unless this is the last step
  // by count it is not stored (8 of the pass's 34 bytes per row); should the stopping test end the loop here after all, one
  // single-stage sweep of the same input reproduces it bit for bit (finish).
  int step_last_sweep(long long count, double* norm) {
    const bool last = count == maxIter || h->opt.no_dead_t;
    if (count == maxIter && spare == x) std::swap(alt, spare);   // the last iterate straight into the caller's buffer: no copy at the end
    double* next = count < maxIter ? spare : nullptr;
    if (ghs) {   // sharded: the residual is stored and its norm taken over the owned rows of all ranks
      MG_TRY(need(cur, 2));
      MG_TRY(need(b, 1));
      for (double* v : {alt, Lr, spare}) MG_TRY(need(v, 0));
      MG_TRY(k_smooth_residual(h, 0, b, cur, last ? alt : nullptr, Lr, next, false));
      if (gh0) {
        const int db = depth(b), dt = std::min(dec(depth(cur)), db), dr = std::min(dec(dt), db);
        if (last) valid_on(alt, dt);
        valid_on(Lr, dr);
        if (next) valid_on(spare, std::min(dt, dr));
      }
      MG_TRY(gh_norm_own(h, Lr, norm));
    } else {
      MG_TRY(k_smooth_residual(h, 0, b, cur, last ? alt : nullptr, nullptr, next, true));
      MG_TRY(scalar_sync(h, norm));
    }
    x1_ready = count < maxIter;
    double* freed = cur;
    cur = alt;
    alt = spare;
    spare = freed;
    t_missing = !last;
    return MG_OK;
  }

  // SolveFuncs.jl:26-30: r = b - A x and ||r|| in one pass; where the kernel allows, the same pass also writes alt = x + d.*r, the
  // first pre-smoothing update of the next cycle (unused if this was the last step)
  int step_residual(long long count, double* norm) {
    if (ghs) {
      MG_TRY(need(cur, 1));
      MG_TRY(need(Lr, 0));
      MG_TRY(k_residual(h, 0, L.A, b, cur, Lr));
      valid_on(Lr, std::min(dec(depth(cur)), depth(b)));
      x1_ready = false;
      return gh_norm_own(h, Lr, norm);
    }
    MG_TRY(k_residual_sumsq(h, 0, L.A, b, cur, Lr, count < maxIter ? alt : nullptr, &x1_ready, /*r_dead=*/true));
    return scalar_sync(h, norm);
  }

  int run(bool x_zero) {
    const bool dbg = h->opt.debug_timing;
    auto tprev = std::chrono::steady_clock::now();
    for (long long count = 1; count <= maxIter; ++count) {
      double* out = nullptr;
      bool deferred = fuse_post;
      // (from the second step on, L.r = b - A*x is the residual just computed for the stopping test)
      MG_TRY(cycle_level(h, 0, b, cur, alt, x_zero, h->cycle, &out, /*r_valid=*/count > 1 || !x_zero, x1_ready, &deferred, false, pre_done));
      if (out != cur) std::swap(cur, alt);
      x_zero = false;
      pre_done = false;
      bool stop = false;
      if (four_stage_serves(count, deferred)) {
        MG_TRY(step_four_stage(count, &stop));
        if (stop) break;
        continue;
      }
      MG_TRY(read_pending(&stop));                  // (a step of another kind: first the pending norm)
      if (stop) { MG_TRY(finish_from_keep()); break; }
      if (keep) { spare = keep; keep = nullptr; }
      double nrm = 0.0;
      if (deferred) MG_TRY(step_last_sweep(count, &nrm));
      else MG_TRY(step_residual(count, &nrm));
      if (dbg) {
        auto tnow = std::chrono::steady_clock::now();
        fprintf(stderr, "[mg] step %lld: %.3f ms\n", count, std::chrono::duration<double, std::milli>(tnow - tprev).count());
        tprev = tnow;
      }
      if (record(nrm)) break;
      t_missing = false;            // (the loop goes on: the iterate of this step is never read)
    }
    return MG_OK;
  }

  // the iterate into the caller's buffer
  int finish(long long* iters) {
    if (!stopped && pending) {     // (the last step by count is never a four-stage step; kept so that no norm is ever left unread)
      bool stop = false;
      MG_TRY(read_pending(&stop));
      MG_TRY(finish_from_keep());
    }
    if (t_missing && !stopped) {   // spare: the input of the last pass; cur: the iterate
      MG_TRY(need(spare, 1));
      MG_TRY(need(cur, 0));
      MG_TRY(k_smooth(h, 0, L.A, L.d.p, b, spare, cur));
    }
    if (cur != x) {
      HIP_TRY(hipMemcpyAsync(x, cur, sizeof(double) * len, hipMemcpyDeviceToDevice, h->play->stream));
      HIP_TRY(spin_sync(h->play->stream));
    }
    if (iters) *iters = it;
    return gh_check_depths(h);
  }
};

int solve_dev(mg_hierarchy* h, const double* b, double* x, double tol, long long maxIter, long long* iters, double* resvec) {
  SolveLoop S(h, b, x, tol, maxIter, resvec);
  bool x_zero = false;
  MG_TRY(S.begin(&x_zero));
  MG_TRY(S.run(x_zero));
  return S.finish(iters);
}

// ---------------------------------------------------------------------------------------------------------------------------
// A block of right-hand sides solved COLUMN BY COLUMN on the single-vector kernels (round 4).  The block kernels (SpMM) exist to
// read the matrix once for all columns; an operator stored as row classes has no matrix stream to share, and its single-vector
// path has the tile forms the block path cannot have (a slab of 16 columns does not fit the LDS): C5 took 9.57 ms per step for 16
// columns where 16 single-vector steps take 7.7.  Every step runs the cycle of every column (the coarse levels' vectors and
// graphs are shared, the fine-level iterates and residuals are per column), then ONE stopping test on the block norm
// sqrt(sum_c ||r_c||^2) (SolveFuncs.jl:26-37 on the block): the same iterates per column as solveMG on that column alone, the
// same step count for all.  Taken when the fine level has the four-stage pass and the cycle has no host decisions inside.
// ---------------------------------------------------------------------------------------------------------------------------
// nullptr: a block is solved column by column; else the first condition that is not met
const char* columns_why_not(const mg_hierarchy* h) {
  if (h->nrhs < 2 || h->nrhs > 24) return "2 to 24 columns";
  if (h->opt.no_columns) return "switched off (MG_NO_COLUMNS)";
  if (h->relax_type != 0 || h->cycle == 'K' || h->coarse_gmres) return "pointwise smoother, V/W/F cycle, direct coarsest solve";
  if (h->nlevels < 2 || !h->play->stream) return "two levels or more on a stream of the handle";
  const Level& L = h->lev[0];
  if (h->opt.no_march2 || h->opt.no_fused_next || h->opt.no_dead_t || h->opt.no_march4) return "the fused passes are switched off";
  if (!gh_agree4(h) || !gh_agree2(h, 0)) return "a rank of the sharded run whose fine level has no four-stage pass";
  if (!L.A.has_rc || !L.A.rc_has_d || L.A.rc_nexc != 0 || L.A.d_bound != L.d.p) return "fine level in row-class form with relaxPrec per class and no exception rows";
  if (!L.A.rc_march3) return "fine level on the two-stage tile form";
  if (!L.A.rc_march4) return "fine level on the four-stage pass";
  if (!(std::max<long long>(1, L.npre) == 2 && std::max<long long>(1, L.npost) >= 1)) return "V(2,*) smoothing";
  return nullptr;
}
bool columns_ok(const mg_hierarchy* h) { return columns_why_not(h) == nullptr; }
int solve_dev_columns(mg_hierarchy* h, const double* b, double* x, double tol, long long maxIter, long long* iters, double* resvec) {
  Level& L = h->lev[0];
  const long long n = L.n, k = h->nrhs, len = n * k, ns = (n + 1) & ~1LL;   // (even stride: every column 16-byte aligned)
  double res = 0.0, res0 = 0.0, xn = 0.0;
  h->last_b = b;
  h->last_x = x;
  // Ghost-layer form (mg_ghost.inc): every column is a vector of this rank's extended fine box; norms are sums over the owned rows
  // of all ranks (taken per column, behind the transposes); one stream (the exchange buffers of a level serve one vector at a time)
  const bool ghs = gh_global_scalars(h);
  const bool gh0 = gh_level(h, 0) != nullptr;
  if (gh0 && gh_level(h, 0)->gmin < 4)
    return fail(MG_ERR_UNSUPPORTED, "ghost-layer form: a block is solved column by column on the four-stage pass, which needs 4 ghost layers on the fine level (%d)", gh_level(h, 0)->gmin);
  auto gdep = [&](const double* v) { return gh_depth(h, 0, v); };
  auto gdec = [&](int d) { return gh_dec(h, 0, d); };
  MG_TRY(gh_begin_block(h));
  bool x_zero = false;
  if (!ghs) {
    // SolveFuncs.jl:14-22 on the block, as solve_dev does
    MG_TRY(norm_sync(h, x, len, &xn));
    x_zero = (xn == 0.0);
    if (x_zero) {
      MG_TRY(norm_sync(h, b, len, &res0));
    } else {
      MG_TRY(k_residual_sumsq(h, 0, L.A, b, x, h->play->r0));
      MG_TRY(scalar_sync(h, &res0));
    }
    if (resvec) resvec[0] = res0;
    if (iters) *iters = 0;
    if (maxIter == 0) return MG_OK;
  }
  for (auto& cb : h->colbuf)
    if (cb.n != (size_t)(ns * k)) {
      MG_TRY(cb.alloc((size_t)(ns * k)));
      HIP_TRY(hipMemsetAsync(cb.p, 0, cb.bytes(), h->play->stream));
    }
  if (h->h_cols_n < k) {
    if (h->h_cols) (void)hipHostFree(h->h_cols);
    h->h_cols = nullptr;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->h_cols), (size_t)k * sizeof(double)));
    h->h_cols_n = k;
  }
  double *colB = h->colbuf[0].p, *colX = h->colbuf[1].p, *colA = h->colbuf[2].p, *colR = h->colbuf[3].p;
  const unsigned tb = (unsigned)((n + 255) / 256);
  const size_t tlds = (size_t)k * 257 * sizeof(double);
  hipLaunchKernelGGL((mgk::block_columns_transpose<true>), dim3(tb), dim3(256), tlds, h->play->stream, b, colB, n, (int)k, ns);
  if (x_zero) HIP_TRY(hipMemsetAsync(colX, 0, (size_t)(ns * k) * sizeof(double), h->play->stream));
  else hipLaunchKernelGGL((mgk::block_columns_transpose<true>), dim3(tb), dim3(256), tlds, h->play->stream, x, colX, n, (int)k, ns);
  HIP_TRY(hipGetLastError());
  if (ghs) {   // SolveFuncs.jl:14-22 on the block: norms over the owned rows of all ranks, column by column
    auto block_norm = [&](const double* cols, double* out) -> int {
      for (long long c = 0; c < k; ++c) MG_TRY(gh_sumsq_own_to_slot(h, cols + c * ns, h->h_cols + c));
      HIP_TRY(spin_sync(h->play->stream));
      double ss = 0.0;
      for (long long c = 0; c < k; ++c) {
        MG_TRY(gh_host_reduce(h, h->h_cols + c));
        ss += h->h_cols[c];
      }
      *out = std::sqrt(ss);
      return MG_OK;
    };
    MG_TRY(block_norm(colX, &xn));
    x_zero = (xn == 0.0);
    if (gh0)
      for (long long c = 0; c < k; ++c) {   // every column of b with all its ghost layers (once per solve), x: owned rows
        gh_set(h, 0, colB + c * ns, 0);
        MG_TRY(gh_need(h, 0, colB + c * ns, GH_FULL));
        gh_set(h, 0, colX + c * ns, x_zero ? GH_FULL : 0);
      }
    if (x_zero) {
      MG_TRY(block_norm(colB, &res0));
    } else {
      Lane lane(h, 0, 1);
      for (long long c = 0; c < k; ++c) {
        if (gh0) MG_TRY(gh_need(h, 0, colX + c * ns, 1));
        MG_TRY(k_residual(h, 0, L.A, colB + c * ns, colX + c * ns, colR + c * ns));
        if (gh0) gh_set(h, 0, colR + c * ns, std::min(gdec(gdep(colX + c * ns)), gdep(colB + c * ns)));
      }
      MG_TRY(block_norm(colR, &res0));
    }
    if (resvec) resvec[0] = res0;
    if (iters) *iters = 0;
    if (maxIter == 0) return MG_OK;
  }
  // More streams: column c plays in lane c mod S, one vector at a time, on that lane's stream (lane 0: the hierarchy's own), its fine
  // residual the column's slice of colR.
  const int S = (h->play->owns_stream && !h->coarse_lu && !h->prof && !h->ghost) ? (int)std::max<long long>(1, std::min<long long>({h->opt.columns_streams, 8LL, k})) : 1;
  while ((int)h->lanes.size() < S - 1) {
    h->lanes.push_back(new Play());
    h->lane_ready.push_back(nullptr);
  }
  for (int si = 0; si < S - 1; ++si) {
    MG_TRY(h->lanes[(size_t)si]->alloc(h, 1, /*fine=*/false));
    if (!h->lane_ready[(size_t)si]) HIP_TRY(hipEventCreateWithFlags(&h->lane_ready[(size_t)si], hipEventDisableTiming));
  }
  // (also the error path: nothing of a column may still be in flight on another lane's stream once this returns)
  struct Drain {
    mg_hierarchy* h;
    ~Drain() {
      for (Play* p : h->lanes)
        if (p->stream) (void)spin_sync(p->stream);
    }
  } drain{h};
  double *cur = colX, *alt = colA;               // (every column makes the same swaps: the columns of a role share an array)
  if (!x_zero && !ghs) {    // (sharded: the residuals of the initial norm are those)
    Lane lane(h, 0, 1);
    for (long long c = 0; c < k; ++c) MG_TRY(k_residual(h, 0, L.A, colB + c * ns, cur + c * ns, colR + c * ns));
  }
  for (int si = 0; si < S - 1; ++si) {   // (the columns of the other lanes wait for the transposes)
    HIP_TRY(hipEventRecord(h->lane_ready[(size_t)si], h->play->stream));
    HIP_TRY(hipStreamWaitEvent(h->lanes[(size_t)si]->stream, h->lane_ready[(size_t)si], 0));
  }
  bool pre_done = false;
  long long it = 0;
  for (long long count = 1; count <= maxIter; ++count) {
    const bool last = count == maxIter;
    bool swapped = false;
    for (long long c = 0; c < k; ++c) {
      const double* bc = colB + c * ns;
      double *xc = cur + c * ns, *ac = alt + c * ns, *rc = colR + c * ns, *out = nullptr;
      Lane lane(h, (int)(c % S), 1, rc);
      bool deferred = true;
      MG_TRY(cycle_level(h, 0, bc, xc, ac, x_zero && count == 1, h->cycle, &out, /*r_valid=*/count > 1 || !x_zero, false, &deferred, false, pre_done));
      if (!deferred) return fail(MG_ERR_STATE, "column-wise solve: the fine level left its last sweep inside the cycle");
      if (c == 0) swapped = out != xc;
      else if (swapped != (out != xc)) return fail(MG_ERR_STATE, "column-wise solve: columns disagree on their buffers");
      double *xin = swapped ? ac : xc, *xout = swapped ? xc : ac;     // xin: x before the last sweep
      if (!last) {
        if (!march4_ok(h, 0, xin, xout, rc)) return fail(MG_ERR_STATE, "column-wise solve: the four-stage pass does not serve the fine level");
        if (gh0) {
          MG_TRY(gh_need(h, 0, xin, 5));
          MG_TRY(gh_need(h, 0, bc, 4));
          MG_TRY(gh_need(h, 0, xout, 0));
          MG_TRY(gh_need(h, 0, rc, 0));
        }
        MG_TRY(k_four_stage(h, 0, bc, xin, xout, rc, h->h_cols + c));       // xout = t', rc = r', ||r_c||^2 of this step
        if (gh0) {
          const int db = gdep(bc), dt = std::min(gdec(gdep(xin)), db), dr = std::min(gdec(dt), db), dn = std::min(dt, dr);
          const int dp = std::min(gdec(dn), db);
          gh_set(h, 0, xout, dp);
          gh_set(h, 0, rc, std::min(gdec(dp), db));
        }
      } else if (ghs) {   // sharded: the residual is stored, its norm taken over the owned rows of all ranks
        if (gh0) {
          MG_TRY(gh_need(h, 0, xin, 2));
          MG_TRY(gh_need(h, 0, bc, 1));
          MG_TRY(gh_need(h, 0, xout, 0));
          MG_TRY(gh_need(h, 0, rc, 0));
        }
        MG_TRY(k_smooth_residual(h, 0, bc, xin, xout, rc, nullptr, false));
        if (gh0) {
          const int db = gdep(bc), dt = std::min(gdec(gdep(xin)), db);
          gh_set(h, 0, xout, dt);
          gh_set(h, 0, rc, std::min(gdec(dt), db));
        }
        MG_TRY(gh_sumsq_own_to_slot(h, rc, h->h_cols + c));
      } else {
        MG_TRY(k_smooth_residual(h, 0, bc, xin, xout, nullptr, nullptr, true));  // xout = the iterate, ||r_c||^2
        HIP_TRY(hipMemcpyAsync(h->h_cols + c, h->play->scalar.p, sizeof(double), hipMemcpyDeviceToHost, h->play->stream));
        h->play->scalar_mirrored = false;   // (the lanes share the pinned slot: read with a copy of its own, it mirrors none of them)
      }
    }
    if (swapped) std::swap(cur, alt);              // cur: x before the last sweep (every column); alt: t' / the iterate
    for (int si = 0; si < S - 1; ++si) HIP_TRY(spin_sync(h->lanes[(size_t)si]->stream));
    HIP_TRY(spin_sync(h->play->stream));
    double ss = 0.0;
    for (long long c = 0; c < k; ++c) {
      if (ghs) MG_TRY(gh_host_reduce(h, h->h_cols + c));   // (host-staged transport: the ranks' sums are added here)
      ss += h->h_cols[c];
    }
    res = std::sqrt(ss);
    ++it;
    if (resvec) resvec[it] = res;
    const bool stop = res / res0 < tol;            // SolveFuncs.jl:34-36
    if (last) { std::swap(cur, alt); break; }      // (the iterate was written)
    if (stop) {                                    // the two speculative stages are dropped: the iterate from the pass's input
      Lane lane(h, 0, 1);
      for (long long c = 0; c < k; ++c) {
        if (gh0) { MG_TRY(gh_need(h, 0, cur + c * ns, 1)); MG_TRY(gh_need(h, 0, alt + c * ns, 0)); }
        MG_TRY(k_smooth(h, 0, L.A, L.d.p, colB + c * ns, cur + c * ns, alt + c * ns));
      }
      std::swap(cur, alt);
      break;
    }
    std::swap(cur, alt);                           // t': the next cycle's x after its pre-smoothing
    pre_done = true;
  }
  hipLaunchKernelGGL((mgk::block_columns_transpose<false>), dim3(tb), dim3(256), tlds, h->play->stream, cur, x, n, (int)k, ns);
  HIP_TRY(hipGetLastError());
  HIP_TRY(spin_sync(h->play->stream));
  if (iters) *iters = it;
  return gh_check_depths(h);
}

// ONE cycle on a block of right-hand sides in the ghost-layer form: column by column on the single-vector kernels (a column is a
// vector of this rank's extended fine box: its ghost layers travel per column, as in solve_dev_columns).  MGdef.jl:163-176.
int cycle_dev_columns(mg_hierarchy* h, const double* b, double* x, bool x_zero) {
  Level& L = h->lev[0];
  const long long n = L.n, k = h->nrhs, ns = (n + 1) & ~1LL;
  for (int i = 0; i < 2; ++i)
    if (h->colbuf[i].n != (size_t)(ns * k)) {
      MG_TRY(h->colbuf[i].alloc((size_t)(ns * k)));
      HIP_TRY(hipMemsetAsync(h->colbuf[i].p, 0, h->colbuf[i].bytes(), h->play->stream));
    }
  double *colB = h->colbuf[0].p, *colX = h->colbuf[1].p;
  const unsigned tb = (unsigned)((n + 255) / 256);
  const size_t tlds = (size_t)k * 257 * sizeof(double);
  hipLaunchKernelGGL((mgk::block_columns_transpose<true>), dim3(tb), dim3(256), tlds, h->play->stream, b, colB, n, (int)k, ns);
  if (x_zero) HIP_TRY(hipMemsetAsync(colX, 0, (size_t)(ns * k) * sizeof(double), h->play->stream));
  else hipLaunchKernelGGL((mgk::block_columns_transpose<true>), dim3(tb), dim3(256), tlds, h->play->stream, x, colX, n, (int)k, ns);
  HIP_TRY(hipGetLastError());
  {
    Lane lane(h, 0, 1);
    for (long long c = 0; c < k; ++c) MG_TRY(cycle_dev(h, colB + c * ns, colX + c * ns, x_zero));
  }
  hipLaunchKernelGGL((mgk::block_columns_transpose<false>), dim3(tb), dim3(256), tlds, h->play->stream, colX, x, n, (int)k, ns);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}

// dot(x,y) on the host; synchronises the stream
int dot_sync(mg_hierarchy* h, const double* x, const double* y, long long len, double* out) {
  const int nb = (int)std::min<long long>(h->nred_blocks, std::max<long long>(1, (len / 2 + mgk::BLK - 1) / mgk::BLK));
  hipLaunchKernelGGL(mgk::dot_partial, dim3(nb), dim3(mgk::BLK), 0, h->play->stream, x, y, len, h->play->partial.p);
  launch_sum_final(h, h->play->partial.p, nb);
  HIP_TRY(hipGetLastError());
  MG_TRY(scalar_wait(h));
  *out = *h->h_scalar;
  return MG_OK;
}

// y = A x on level `level` and *out = x'y: where the marching kernel serves the product its per-workgroup partials are of
// x[row]*y[row] (VecArgs::dotx), else the product and a dot pass.  Synchronises the stream.
int k_spmv_dot(mg_hierarchy* h, int level, const Csr& A, const double* x, double* y, double* out) {
  mgk::VecArgs v{};
  v.x = x;
  v.y = y;
  v.alpha = 1.0;
  v.beta = 0.0;
  v.nrhs = (int)h->play->nrhs;
  if (h->play->nrhs == 1 && march_ok(A, v) && A.rc_nexc == 0 && (size_t)A.rm_nblocks <= h->play->partial.n) {
    v.sumsq = h->play->partial.p;
    v.dotx = 1;
    int nb1 = 0;
    {
      ProfScope ps(h, level, MG_K_SPMV, spmv_bytes(A, 1, false, false), moved_bytes(A, 1, false, false));
      MG_TRY(launch_csr<mgk::AXPBY>(h->play->stream, A, v, &nb1));
    }
    launch_sum_final(h, h->play->partial.p, nb1);
    HIP_TRY(hipGetLastError());
    MG_TRY(scalar_wait(h));
    *out = *h->h_scalar;
    return MG_OK;
  }
  MG_TRY(k_spmv(h, level, MG_K_SPMV, A, 1.0, x, 0.0, y));
  return dot_sync(h, x, y, (long long)A.n_rows * h->play->nrhs, out);
}

}  // namespace
