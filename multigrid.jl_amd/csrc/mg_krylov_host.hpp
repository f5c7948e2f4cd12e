// mg_krylov_host.hpp - the small HOST algebra of the Krylov drivers (mg_krylov.inc, mg_dist_krylov.inc, mg_complex_krylov.inc) and of the
// FGMRES relaxation (mg_schedule.inc, mg_dist.inc).  Plain C++17 with no HIP header: mgvcycle.hip includes it in front of its parts, and
// tests/native/krylov_host_algebra.cpp builds it on its own.  Nothing here touches a device vector.
//   KrylovReport        where a driver writes iters / flag / resvec / nres, and its epilogue
//   HessenbergLsq<S>    the Givens least squares of FGMRES(m), S = double or std::complex<double>
//   coarse_gmres_replay the replay of a complex hierarchy's GMRES coarsest solve from its table of scalars
//   coarse_block_gmres_replay, BlockHessenbergLsq   the same for a block of right-hand sides (at the end)
//   pinv_sym, RelaxLsq  the normal-equations step of FGMRES_relaxation (Jac-GMRES smoother, K-cycle)
//   RelaxLsqC           the same for ComplexF64 hierarchies: Hermitian H, solved on its leading blocks
//   SmallMatT<S>, sm_*  row-major dense helpers of the block drivers, S = double (SmallMat) or std::complex<double>
#pragma once

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstddef>
#include <utility>
#include <vector>

// ---- a driver's outputs: any pointer may be null ----------------------------------------------------------------------------------
struct KrylovReport {
  long long* iters = nullptr;
  long long* flag = nullptr;
  double* resvec = nullptr;
  long long* nres = nullptr;
  long long nr = 0;   // entries appended so far
  KrylovReport(long long* iters_, long long* flag_, double* resvec_, long long* nres_) : iters(iters_), flag(flag_), resvec(resvec_), nres(nres_) {}
  void record(double err) {
    if (resvec) resvec[nr] = err;
    ++nr;
  }
  // indexed, not appended: PCG's one entry per iteration (and the halo form's later overwrite of it); nres does not count these
  void set(long long k, double err) {
    if (resvec) resvec[k] = err;
  }
  int finish(long long it, long long f) {
    if (iters) *iters = it;
    if (flag) *flag = f;
    if (nres) *nres = nr;
    return 0;   // MG_OK
  }
};

// ---- FGMRES(m): min || beta e_1 - Hbar y || by Givens rotations, column by column -------------------------------------------------
// Column i holds h_0 .. h_i (S) and the real h_{i+1,i} = ||w||.  Its rotation has a cosine of type S and a real sine:
//   rr = radius(a, b), c = a / rr, s = b / rr with a = h_i (rotated by the columns before it), b = h_{i+1,i}; rr == 0: c = 1, s = 0.
inline double krylov_conj(double a) { return a; }
inline std::complex<double> krylov_conj(const std::complex<double>& a) { return std::conj(a); }
inline double krylov_radius(double a, double b) { return std::hypot(a, b); }
inline double krylov_radius(const std::complex<double>& a, double b) { return std::sqrt(std::norm(a) + b * b); }
inline double krylov_abs(double a) { return std::fabs(a); }
inline double krylov_abs(const std::complex<double>& a) { return std::abs(a); }

template <class S>
struct HessenbergLsq {
  const int m;
  std::vector<S> H, cs, s, y;     // H: m x m, row-major (rotated columns are upper triangular); s: the rotated right-hand side
  std::vector<double> sn, sub;    // sines; sub[i] = h_{i+1,i} as the Arnoldi step left it
  explicit HessenbergLsq(int m_)
      : m(m_), H((size_t)m_ * m_, S(0.0)), cs((size_t)m_, S(0.0)), s((size_t)m_ + 1, S(0.0)), y((size_t)m_, S(0.0)), sn((size_t)m_, 0.0), sub((size_t)m_, 0.0) {}
  void begin(double rnorm) {      // a restart: s = ||r|| e_1
    std::fill(s.begin(), s.end(), S(0.0));
    s[0] = rnorm;
  }
  S& h(int k, int i) { return H[(size_t)k * m + i]; }      // k <= i
  double& hsub(int i) { return sub[(size_t)i]; }
  // rotates column i and the right-hand side; returns |s_{i+1}|, the residual norm of the least squares over columns 0 .. i
  double close_column(int i) {
    for (int k = 0; k < i; ++k) {                           // previous rotations
      const S t = krylov_conj(cs[(size_t)k]) * h(k, i) + sn[(size_t)k] * h(k + 1, i);
      h(k + 1, i) = -sn[(size_t)k] * h(k, i) + cs[(size_t)k] * h(k + 1, i);
      h(k, i) = t;
    }
    const S a = h(i, i);
    const double bq = sub[(size_t)i];
    const double rr = krylov_radius(a, bq);
    cs[(size_t)i] = (rr == 0.0) ? S(1.0) : a / rr;
    sn[(size_t)i] = (rr == 0.0) ? 0.0 : bq / rr;
    h(i, i) = rr;
    s[(size_t)i + 1] = -sn[(size_t)i] * s[(size_t)i];
    s[(size_t)i] = krylov_conj(cs[(size_t)i]) * s[(size_t)i];
    return krylov_abs(s[(size_t)i + 1]);
  }
  const std::vector<S>& solve(int used) {
    for (int i = used - 1; i >= 0; --i) {                   // y = H \ s (upper triangular)
      S acc = s[(size_t)i];
      for (int k = i + 1; k < used; ++k) acc -= h(i, k) * y[(size_t)k];
      y[(size_t)i] = acc / h(i, i);
    }
    return y;
  }
};

// ---- the GMRES coarsest solve of a complex hierarchy (mg_complex.inc: cx_coarse_gmres): the host's replay of ONE restart of
// FGMRES(m) from x = 0 that the device has run to its end.  tab: tab[0] = ||b||^2; column i from slot(i) = 1 + i^2 + 2 i on:
// h_0 .. h_i (re, im each), then ||w||^2 - (m + 1)^2 doubles for m columns.  The columns are closed one after the other and the
// loop breaks at the first err / ||b|| <= tol (KrylovMethods.fgmres); columns behind the break are not read.  used: the columns that
// enter x = Z[:, :used] y (Q.solve(used) has run; y = Q.y); flag 0 (the estimate met tol), -1 (it did not), -9 (b = 0: x = 0, used = 0);
// resvec[i] = err_i / ||b|| for i < used.
inline int coarse_gmres_slot(int i) { return 1 + i * i + 2 * i; }
inline void coarse_gmres_replay(const double* tab, double tol, HessenbergLsq<std::complex<double>>& Q, int& used, long long& flag,
                                double* resvec) {
  used = 0;
  flag = -1;
  if (!(tab[0] > 0.0)) {
    flag = -9;
    return;
  }
  const double bn = std::sqrt(tab[0]);
  Q.begin(bn);
  for (int i = 0; i < Q.m; ++i) {
    const double* c = tab + coarse_gmres_slot(i);
    for (int k = 0; k <= i; ++k) Q.h(k, i) = std::complex<double>(c[2 * k], c[2 * k + 1]);
    Q.hsub(i) = std::sqrt(c[2 * (i + 1)]);
    const double err = Q.close_column(i) / bn;
    if (resvec) resvec[i] = err;
    used = i + 1;
    if (err <= tol) {
      flag = 0;
      break;
    }
  }
  Q.solve(used);
}

// ---- FGMRES_relaxation (FGMRES.jl:48-126): the normal equations of min || r0 - A Z t || ---------------------------------------------
// Moore-Penrose inverse of a small symmetric matrix (H = (AZ)'(AZ), k <= 16) by cyclic Jacobi rotations;
// cut-off as Julia's pinv: rtol = eps * k relative to the largest singular value.
// kcut: the order that enters the cut-off where H is a leading block (or an embedding) of a larger zero-padded matrix; 0: k itself.
inline void pinv_sym(const std::vector<double>& H, int k, std::vector<double>& Pinv, int kcut = 0) {
  std::vector<double> A(H), V((size_t)k * k, 0.0);
  for (int i = 0; i < k; ++i) V[(size_t)i * k + i] = 1.0;
  for (int sweep = 0; sweep < 100; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < k; ++p)
      for (int q = p + 1; q < k; ++q) off += A[(size_t)p * k + q] * A[(size_t)p * k + q];
    if (off < 1e-300) break;
    for (int p = 0; p < k; ++p)
      for (int q = p + 1; q < k; ++q) {
        const double apq = A[(size_t)p * k + q];
        if (apq == 0.0) continue;
        const double theta = (A[(size_t)q * k + q] - A[(size_t)p * k + p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
        for (int i = 0; i < k; ++i) {
          const double aip = A[(size_t)i * k + p], aiq = A[(size_t)i * k + q];
          A[(size_t)i * k + p] = c * aip - sn * aiq;
          A[(size_t)i * k + q] = sn * aip + c * aiq;
        }
        for (int i = 0; i < k; ++i) {
          const double api = A[(size_t)p * k + i], aqi = A[(size_t)q * k + i];
          A[(size_t)p * k + i] = c * api - sn * aqi;
          A[(size_t)q * k + i] = sn * api + c * aqi;
        }
        for (int i = 0; i < k; ++i) {
          const double vip = V[(size_t)i * k + p], viq = V[(size_t)i * k + q];
          V[(size_t)i * k + p] = c * vip - sn * viq;
          V[(size_t)i * k + q] = sn * vip + c * viq;
        }
      }
  }
  double smax = 0.0;
  for (int i = 0; i < k; ++i) smax = std::max(smax, std::fabs(A[(size_t)i * k + i]));
  const double tol = 2.220446049250313e-16 * (kcut > 0 ? kcut : k) * smax;
  Pinv.assign((size_t)k * k, 0.0);
  for (int e = 0; e < k; ++e) {
    const double lam = A[(size_t)e * k + e];
    if (std::fabs(lam) <= tol) continue;
    for (int i = 0; i < k; ++i)
      for (int j = 0; j < k; ++j) Pinv[(size_t)i * k + j] += V[(size_t)i * k + e] * V[(size_t)j * k + e] / lam;
  }
}

// H = (AZ)'(AZ) and xi = (AZ)'r0 grow by one direction per step (the rest stays zero); step() gives t = pinv(H) xi over all k and the
// residual estimate rn = sqrt(|t'Ht - 2 t'xi + ||r0||^2|).
struct RelaxLsq {
  const int k;
  std::vector<double> H, xi, tv, Pinv;
  explicit RelaxLsq(int k_) : k(k_), H((size_t)k_ * k_, 0.0), xi((size_t)k_, 0.0), tv((size_t)k_, 0.0) {}
  void set(int i, int j, double d) {                                       // H[:,j] = t; H[j,:] = t'  (l.99-101)
    H[(size_t)i * k + j] = d;
    H[(size_t)j * k + i] = d;
  }
  const std::vector<double>& t() const { return tv; }
  double step(double rnorm0) {
    pinv_sym(H, k, Pinv);                                                  // t = pinv(H)*xi           (l.102)
    double tHt = 0.0, txi = 0.0;
    for (int a = 0; a < k; ++a) {
      double s = 0.0;
      for (int b = 0; b < k; ++b) s += Pinv[(size_t)a * k + b] * xi[(size_t)b];
      tv[(size_t)a] = s;
    }
    for (int a = 0; a < k; ++a) {
      double s = 0.0;
      for (int b = 0; b < k; ++b) s += H[(size_t)a * k + b] * tv[(size_t)b];
      tHt += tv[(size_t)a] * s;
      txi += tv[(size_t)a] * xi[(size_t)a];
    }
    return std::sqrt(std::fabs(tHt - 2.0 * txi + rnorm0 * rnorm0));       // l.104
  }
};

// The same for VAL = ComplexF64 (mg_complex.inc: cx_fgmres_relax, the K-cycle of cx_cycle): H = (AZ)'(AZ) is Hermitian and xi complex
// (Julia's dot conjugates its first argument).  The device hands over ALL Gram scalars of a relaxation at once, so step(m, .) solves on
// the leading m x m block - the reference's pinv of its zero-padded k x k H gives the same t with zeros behind it, cut-off
// eps * k * sigma_max included.  The Moore-Penrose inverse comes from pinv_sym on the real symmetric embedding [Re H, -Im H; Im H, Re H]
// (every eigenvalue of H twice, the inverse of the embedding is the embedding of the inverse).
struct RelaxLsqC {
  typedef std::complex<double> zc;
  const int k;
  std::vector<zc> H, xi, tv;
  explicit RelaxLsqC(int k_) : k(k_), H((size_t)k_ * k_, zc(0.0)), xi((size_t)k_, zc(0.0)), tv((size_t)k_, zc(0.0)) {}
  // column j of t = AZ' w, entry i <= j:  H[:,j] = t; H[j,:] = t'; H = (H + H')/2  (l.99-101: the diagonal comes out real)
  void set(int i, int j, zc d) {
    if (i == j) {
      H[(size_t)j * k + j] = zc(d.real(), 0.0);
    } else {
      H[(size_t)i * k + j] = d;
      H[(size_t)j * k + i] = std::conj(d);
    }
  }
  const std::vector<zc>& t() const { return tv; }
  // t = pinv(H[:m,:m]) xi[:m] (zero behind m); returns rn = sqrt(|Re(t'Ht - 2 t'xi + ||r0||^2)|)   (l.102-104)
  double step(int m, double rnorm0) {
    const int e = 2 * m;
    std::vector<double> E((size_t)e * e, 0.0), Pinv;
    for (int a = 0; a < m; ++a)
      for (int b = 0; b < m; ++b) {
        const zc h = H[(size_t)a * k + b];
        E[(size_t)a * e + b] = h.real();
        E[(size_t)(a + m) * e + b + m] = h.real();
        E[(size_t)a * e + b + m] = -h.imag();
        E[(size_t)(a + m) * e + b] = h.imag();
      }
    pinv_sym(E, e, Pinv, k);
    std::fill(tv.begin(), tv.end(), zc(0.0));
    for (int a = 0; a < m; ++a) {
      double re = 0.0, im = 0.0;
      for (int b = 0; b < m; ++b) {
        re += Pinv[(size_t)a * e + b] * xi[(size_t)b].real() + Pinv[(size_t)a * e + b + m] * xi[(size_t)b].imag();
        im += Pinv[(size_t)(a + m) * e + b] * xi[(size_t)b].real() + Pinv[(size_t)(a + m) * e + b + m] * xi[(size_t)b].imag();
      }
      tv[(size_t)a] = zc(re, im);
    }
    zc tHt(0.0), txi(0.0);
    for (int a = 0; a < m; ++a) {
      zc s(0.0);
      for (int b = 0; b < m; ++b) s += H[(size_t)a * k + b] * tv[(size_t)b];
      tHt += std::conj(tv[(size_t)a]) * s;
      txi += std::conj(tv[(size_t)a]) * xi[(size_t)a];
    }
    return std::sqrt(std::fabs((tHt - 2.0 * txi).real() + rnorm0 * rnorm0));
  }
};

// ---- dense helpers of the block drivers ---------------------------------------------------------------------------------------------
// (S = double: the real block drivers; S = std::complex<double>: the complex block drivers of mg_complex_krylov.inc - block BiCGSTAB
// uses sm_mul, sm_solve and sm_scaled_identity, block FGMRES sm_mul and the complex sm_chol_semidefinite, sm_tri_pinv, sm_lstsq)
template <class S>
struct SmallMatT {   // row-major dense helper, host
  int r = 0, c = 0;
  std::vector<S> a;
  SmallMatT() {}
  SmallMatT(int r_, int c_) : r(r_), c(c_), a((size_t)r_ * c_, S(0.0)) {}
  S& operator()(int i, int j) { return a[(size_t)i * c + j]; }
  S operator()(int i, int j) const { return a[(size_t)i * c + j]; }
};
typedef SmallMatT<double> SmallMat;
template <class S>
inline SmallMatT<S> sm_mul(const SmallMatT<S>& A, const SmallMatT<S>& B) {
  SmallMatT<S> C(A.r, B.c);
  for (int i = 0; i < A.r; ++i)
    for (int k = 0; k < A.c; ++k) {
      const S v = A(i, k);
      for (int j = 0; j < B.c; ++j) C(i, j) += v * B(k, j);
    }
  return C;
}
inline SmallMat sm_T(const SmallMat& A) {
  SmallMat C(A.c, A.r);
  for (int i = 0; i < A.r; ++i)
    for (int j = 0; j < A.c; ++j) C(j, i) = A(i, j);
  return C;
}
// X = A \ B by Gaussian elimination with partial pivoting (A k x k; pivots by modulus); false if singular
template <class S>
inline bool sm_solve(SmallMatT<S> A, SmallMatT<S> B, SmallMatT<S>& X) {
  const int k = A.r;
  for (int p = 0; p < k; ++p) {
    int piv = p;
    for (int i = p + 1; i < k; ++i)
      if (krylov_abs(A(i, p)) > krylov_abs(A(piv, p))) piv = i;
    if (A(piv, p) == S(0.0)) return false;
    if (piv != p) {
      for (int j = 0; j < k; ++j) std::swap(A(p, j), A(piv, j));
      for (int j = 0; j < B.c; ++j) std::swap(B(p, j), B(piv, j));
    }
    for (int i = p + 1; i < k; ++i) {
      const S f = A(i, p) / A(p, p);
      if (f == S(0.0)) continue;
      for (int j = p; j < k; ++j) A(i, j) -= f * A(p, j);
      for (int j = 0; j < B.c; ++j) B(i, j) -= f * B(p, j);
    }
  }
  X = SmallMatT<S>(k, B.c);
  for (int j = 0; j < B.c; ++j)
    for (int i = k - 1; i >= 0; --i) {
      S acc = B(i, j);
      for (int t = i + 1; t < k; ++t) acc -= A(i, t) * X(t, j);
      X(i, j) = acc / A(i, i);
    }
  return true;
}
// upper triangular Rf with G = Rf'Rf for a positive SEMI-definite Gram matrix
inline SmallMat sm_chol_semidefinite(const SmallMat& G, double rtol = 1e-14) {
  const int k = G.r;
  SmallMat R(k, k);
  for (int c = 0; c < k; ++c) {
    double d = G(c, c);
    for (int a = 0; a < c; ++a) d -= R(a, c) * R(a, c);
    if (G(c, c) <= 0.0 || d <= rtol * G(c, c)) continue;
    R(c, c) = std::sqrt(d);
    for (int j = c + 1; j < k; ++j) {
      double t = G(c, j);
      for (int a = 0; a < c; ++a) t -= R(a, c) * R(a, j);
      R(c, j) = t / R(c, c);
    }
  }
  return R;
}
// T with W*T = W*Rf^+: T[:,c] = (e_c - T[:,:c] Rf[:c,c]) / Rf[c,c], zero for zero pivots
inline SmallMat sm_tri_pinv(const SmallMat& R) {
  const int k = R.r;
  SmallMat T(k, k);
  for (int c = 0; c < k; ++c) {
    if (R(c, c) == 0.0) continue;
    for (int i = 0; i < k; ++i) {
      double t = (i == c) ? 1.0 : 0.0;
      for (int a = 0; a < c; ++a) t -= T(i, a) * R(a, c);
      T(i, c) = t / R(c, c);
    }
  }
  return T;
}
// min || xi - H Y ||_F over Y by Householder QR of H (rows x cols, rows >= cols); returns the residual norm
inline double sm_lstsq(SmallMat H, SmallMat xi, SmallMat& Y) {
  const int m = H.r, n = H.c, k = xi.c;
  for (int j = 0; j < n; ++j) {
    double nrm = 0.0;
    for (int i = j; i < m; ++i) nrm += H(i, j) * H(i, j);
    nrm = std::sqrt(nrm);
    if (nrm == 0.0) continue;
    const double alpha = H(j, j) > 0 ? -nrm : nrm;
    std::vector<double> v((size_t)m, 0.0);
    for (int i = j; i < m; ++i) v[(size_t)i] = H(i, j);
    v[(size_t)j] -= alpha;
    double vn = 0.0;
    for (int i = j; i < m; ++i) vn += v[(size_t)i] * v[(size_t)i];
    if (vn == 0.0) continue;
    for (int c = j; c < n; ++c) {
      double d = 0.0;
      for (int i = j; i < m; ++i) d += v[(size_t)i] * H(i, c);
      d *= 2.0 / vn;
      for (int i = j; i < m; ++i) H(i, c) -= d * v[(size_t)i];
    }
    for (int c = 0; c < k; ++c) {
      double d = 0.0;
      for (int i = j; i < m; ++i) d += v[(size_t)i] * xi(i, c);
      d *= 2.0 / vn;
      for (int i = j; i < m; ++i) xi(i, c) -= d * v[(size_t)i];
    }
  }
  Y = SmallMat(n, k);
  for (int c = 0; c < k; ++c)
    for (int i = n - 1; i >= 0; --i) {
      double acc = xi(i, c);
      for (int t = i + 1; t < n; ++t) acc -= H(i, t) * Y(t, c);
      Y(i, c) = (H(i, i) != 0.0) ? acc / H(i, i) : 0.0;
    }
  double res = 0.0;
  for (int i = n; i < m; ++i)
    for (int c = 0; c < k; ++c) res += xi(i, c) * xi(i, c);
  return std::sqrt(res);
}
// The same three for S = std::complex<double> (the complex block FGMRES of mg_complex_krylov.inc).  G is Hermitian with a real
// diagonal and G = Rf^H Rf; the pivot rule is the real form's on that real diagonal, d <= rtol * G[c][c].  sm_lstsq reflects with
// I - 2 v v^H / (v^H v), v = x + phase(x_0) ||x|| e_0, which leaves a complex diagonal in the triangular factor.
typedef SmallMatT<std::complex<double>> SmallMatC;
inline SmallMatC sm_chol_semidefinite(const SmallMatC& G, double rtol = 1e-14) {
  typedef std::complex<double> zc;
  const int k = G.r;
  SmallMatC R(k, k);
  for (int c = 0; c < k; ++c) {
    const double g = G(c, c).real();
    double d = g;
    for (int a = 0; a < c; ++a) d -= std::norm(R(a, c));
    if (g <= 0.0 || d <= rtol * g) continue;
    const double rc = std::sqrt(d);
    R(c, c) = zc(rc, 0.0);
    for (int j = c + 1; j < k; ++j) {
      zc t = G(c, j);
      for (int a = 0; a < c; ++a) t -= std::conj(R(a, c)) * R(a, j);
      R(c, j) = t / rc;
    }
  }
  return R;
}
inline SmallMatC sm_tri_pinv(const SmallMatC& R) {
  typedef std::complex<double> zc;
  const int k = R.r;
  SmallMatC T(k, k);
  for (int c = 0; c < k; ++c) {
    if (R(c, c) == zc(0.0)) continue;
    for (int i = 0; i < k; ++i) {
      zc t = (i == c) ? zc(1.0) : zc(0.0);
      for (int a = 0; a < c; ++a) t -= T(i, a) * R(a, c);
      T(i, c) = t / R(c, c);
    }
  }
  return T;
}
inline double sm_lstsq(SmallMatC H, SmallMatC xi, SmallMatC& Y) {
  typedef std::complex<double> zc;
  const int m = H.r, n = H.c, k = xi.c;
  std::vector<zc> v((size_t)m, zc(0.0));
  for (int j = 0; j < n; ++j) {
    double nrm = 0.0;
    for (int i = j; i < m; ++i) nrm += std::norm(H(i, j));
    nrm = std::sqrt(nrm);
    if (nrm == 0.0) continue;
    const double a0 = std::abs(H(j, j));
    const zc alpha = (a0 > 0.0) ? -(H(j, j) / a0) * nrm : zc(-nrm, 0.0);
    for (int i = j; i < m; ++i) v[(size_t)i] = H(i, j);
    v[(size_t)j] -= alpha;
    double vn = 0.0;
    for (int i = j; i < m; ++i) vn += std::norm(v[(size_t)i]);
    if (vn == 0.0) continue;
    for (int c = j; c < n; ++c) {
      zc d(0.0);
      for (int i = j; i < m; ++i) d += std::conj(v[(size_t)i]) * H(i, c);
      d *= 2.0 / vn;
      for (int i = j; i < m; ++i) H(i, c) -= d * v[(size_t)i];
    }
    for (int c = 0; c < k; ++c) {
      zc d(0.0);
      for (int i = j; i < m; ++i) d += std::conj(v[(size_t)i]) * xi(i, c);
      d *= 2.0 / vn;
      for (int i = j; i < m; ++i) xi(i, c) -= d * v[(size_t)i];
    }
  }
  Y = SmallMatC(n, k);
  for (int c = 0; c < k; ++c)
    for (int i = n - 1; i >= 0; --i) {
      zc acc = xi(i, c);
      for (int t = i + 1; t < n; ++t) acc -= H(i, t) * Y(t, c);
      Y(i, c) = (H(i, i) != zc(0.0)) ? acc / H(i, i) : zc(0.0);
    }
  double res = 0.0;
  for (int i = n; i < m; ++i)
    for (int c = 0; c < k; ++c) res += std::norm(xi(i, c));
  return std::sqrt(res);
}
template <class S>
inline SmallMatT<S> sm_scaled_identity(int k, S v) {
  SmallMatT<S> I(k, k);
  for (int i = 0; i < k; ++i) I(i, i) = v;
  return I;
}

// ---- the block GMRES coarsest solve of a complex hierarchy (mg_complex.inc: cx_coarse_block_gmres): the host's replay of ONE restart
// of blockFGMRES(m) from X = 0 that the device has run to its end.  The table (doubles): tab[0] = ||B||_F^2, tab[1] unused, then k x k
// complex blocks, row-major, (re, im) interleaved: block 0 = xi_0, and step j from block coarse_block_slot(j) on: H_0j .. H_jj, H_{j+1,j}.
// BlockHessenbergLsq solves the exact block least squares min ||xi - H Y||_F step by step: the Householder reflections of sm_lstsq
// (the same reflectors: I - 2 v v^H / (v^H v), v = x + phase(x_0) ||x|| e_0), kept between the steps and cut to the k + 1 rows a column
// of a block upper Hessenberg matrix with triangular sub-diagonal blocks reaches - sm_lstsq on the leading blocks adds exact zeros to
// the same sums.  The replay breaks at the first err = ||xi - H Y||_F / ||B||_F <= tol; blocks behind the break are not read.
// used: the steps that enter X = sum_{j < used} Z_j Y_j (Y: (used k) x k); flag 0 / -1, and -9 with used = 0 for B = 0.
inline size_t coarse_block_slot(int j) { return 1 + (size_t)j * ((size_t)j + 3) / 2; }
inline size_t coarse_block_table_len(int k, int m) { return 2 + 2 * (size_t)k * k * coarse_block_slot(m); }   // doubles
struct BlockHessenbergLsq {
  typedef std::complex<double> zc;
  const int k, m, rows;
  // H ((m + 1) k x m k, triangularised column by column) and xi ((m + 1) k x k), both stored COLUMN by column: a reflection works
  // on k + 1 consecutive values of a column (row-major, every step of it would be a cache line of its own)
  std::vector<zc> Hc, xc;
  std::vector<std::vector<zc>> v;      // the reflector of column c: rows c .. c + v[c].size() - 1
  std::vector<double> vn;              // v^H v (0: no reflection)
  BlockHessenbergLsq(int k_, int m_)
      : k(k_), m(m_), rows((m_ + 1) * k_), Hc((size_t)(m_ + 1) * k_ * m_ * k_, zc(0.0)), xc((size_t)(m_ + 1) * k_ * k_, zc(0.0)), v((size_t)m_ * k_),
        vn((size_t)m_ * k_, 0.0) {}
  zc& H(int i, int j) { return Hc[(size_t)j * rows + i]; }
  zc H(int i, int j) const { return Hc[(size_t)j * rows + i]; }
  zc& xi(int i, int j) { return xc[(size_t)j * rows + i]; }
  zc xi(int i, int j) const { return xc[(size_t)j * rows + i]; }
  void begin(const SmallMatC& xi0) {
    std::fill(Hc.begin(), Hc.end(), zc(0.0));
    std::fill(xc.begin(), xc.end(), zc(0.0));
    for (int a = 0; a < k; ++a)
      for (int b = 0; b < k; ++b) xi(a, b) = xi0(a, b);
  }
  // (products written out in real arithmetic: std::complex's operator* goes through the library's NaN-recovering multiply, several
  //  times the cost of the four multiplications, and this runs once per cycle on the critical path)
  static zc mul(const zc& a, const zc& b) { return zc(a.real() * b.real() - a.imag() * b.imag(), a.real() * b.imag() + a.imag() * b.real()); }
  static zc mulc(const zc& a, const zc& b) { return zc(a.real() * b.real() + a.imag() * b.imag(), a.real() * b.imag() - a.imag() * b.real()); }   // conj(a) b
  void reflect(int c, zc* column) const {   // on one column of H or xi
    const std::vector<zc>& w = v[(size_t)c];
    if (vn[(size_t)c] == 0.0) return;
    zc* x = column + c;
    zc d(0.0);
    for (size_t i = 0; i < w.size(); ++i) d += mulc(w[i], x[i]);
    d *= 2.0 / vn[(size_t)c];
    for (size_t i = 0; i < w.size(); ++i) x[i] -= mul(d, w[i]);
  }
  // block column j of H is in place (rows 0 .. (j + 2) k - 1); returns ||xi - H Y||_F over the block columns 0 .. j
  double close_block(int j) {
    const int c0 = j * k, c1 = c0 + k, rlim = (j + 2) * k;
    for (int col = c0; col < c1; ++col)
      for (int c = 0; c < c0; ++c) reflect(c, &Hc[(size_t)col * rows]);
    for (int c = c0; c < c1; ++c) {
      const int hi = std::min(c + k + 1, rlim);
      std::vector<zc>& w = v[(size_t)c];
      w.assign((size_t)(hi - c), zc(0.0));
      vn[(size_t)c] = 0.0;
      double nrm = 0.0;
      for (int i = c; i < hi; ++i) nrm += std::norm(H(i, c));
      nrm = std::sqrt(nrm);
      if (nrm == 0.0) continue;
      const double a0 = std::abs(H(c, c));
      const zc alpha = (a0 > 0.0) ? -(H(c, c) / a0) * nrm : zc(-nrm, 0.0);
      for (int i = c; i < hi; ++i) w[(size_t)(i - c)] = H(i, c);
      w[0] -= alpha;
      double s = 0.0;
      for (const zc& e : w) s += std::norm(e);
      if (s == 0.0) continue;
      vn[(size_t)c] = s;
      for (int col = c; col < c1; ++col) reflect(c, &Hc[(size_t)col * rows]);
      for (int col = 0; col < k; ++col) reflect(c, &xc[(size_t)col * rows]);
    }
    double res = 0.0;
    for (int i = c1; i < rlim; ++i)
      for (int col = 0; col < k; ++col) res += std::norm(xi(i, col));
    return std::sqrt(res);
  }
  // Y = H[:n, :n] \ xi[:n], n = used k, by column-oriented back substitution (row-major (used k) x k, as cb_combine reads it)
  SmallMatC solve(int used) const {
    const int n = used * k;
    SmallMatC Y(n, k);
    std::vector<zc> x((size_t)n);
    for (int c = 0; c < k; ++c) {
      for (int i = 0; i < n; ++i) x[(size_t)i] = xi(i, c);
      for (int i = n - 1; i >= 0; --i) {
        const zc y = (H(i, i) != zc(0.0)) ? x[(size_t)i] / H(i, i) : zc(0.0);
        Y(i, c) = y;
        const zc* hcol = &Hc[(size_t)i * rows];
        for (int r = 0; r < i; ++r) x[(size_t)r] -= mul(hcol[r], y);
      }
    }
    return Y;
  }
};
inline void coarse_block_gmres_replay(const double* tab, int k, double tol, BlockHessenbergLsq& Q, int& used, long long& flag, double* resvec,
                                      SmallMatC& Y) {
  typedef std::complex<double> zc;
  used = 0;
  flag = -1;
  Y = SmallMatC(0, k);
  if (!(tab[0] > 0.0)) {
    flag = -9;
    return;
  }
  const double bn = std::sqrt(tab[0]);
  const size_t kk = (size_t)k * k;
  auto blockat = [&](size_t s, int a, int b) { const double* e = tab + 2 + 2 * (s * kk + (size_t)a * k + b); return zc(e[0], e[1]); };
  SmallMatC xi0(k, k);
  for (int a = 0; a < k; ++a)
    for (int b = 0; b < k; ++b) xi0(a, b) = blockat(0, a, b);
  Q.begin(xi0);
  for (int j = 0; j < Q.m; ++j) {
    const size_t s0 = coarse_block_slot(j);
    for (int i = 0; i <= j + 1; ++i)
      for (int a = 0; a < k; ++a)
        for (int b = 0; b < k; ++b) Q.H(i * k + a, j * k + b) = blockat(s0 + (size_t)i, a, b);
    const double err = Q.close_block(j) / bn;
    if (resvec) resvec[j] = err;
    used = j + 1;
    if (err <= tol) {
      flag = 0;
      break;
    }
  }
  Y = Q.solve(used);
}
