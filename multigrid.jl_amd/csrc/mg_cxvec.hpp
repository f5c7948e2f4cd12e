// mg_cxvec.hpp - fused ComplexF64 vector kernels of the complex Krylov drivers (mg_complex_krylov.inc): one pass over the vectors
// of an update that also leaves the partial sums of the scalars due at that point of the iteration.  The complex counterpart of
// mg_krvec.hpp, whose reduction (mgkv::wave_sum, mgkv::krv_final) and geometry constants it shares.
//
// Shape of every kernel (cxv_pass<Op>): a grid-stride loop over complex elements - one value is one double2, so every vector costs
// one 16-byte load / store per lane and trip.  Vectors must start on a 16-byte boundary (the launchers refuse anything else).  Sums:
// per lane in registers, per wavefront by DPP row operations (no LDS), the 4 wavefronts of a workgroup through 32 bytes of LDS per
// scalar, one partial per workgroup and scalar in HBM (partial[c * gridDim.x + block]); mgkv::krv_final adds them up, one workgroup per
// scalar.  No floating-point atomics anywhere: the grid is a function of n alone, so a rerun adds the same numbers in the same order
// and gives the same bits.
//
// Arithmetic.  A dot is Julia's: dot(a, b) = sum conj(a_i) b_i.  A complex product is the plain four-multiply form (mgk::cmul); an
// update is written as its textbook expression - the product first, then the sum - so FMA contraction can drop roundings but never
// changes which partial results exist (tests/test_complex_krylov_gpu.py counts the roundings of exactly these expressions).
#pragma once
#include "mg_complex.hpp"
#include "mg_krvec.hpp"

namespace mgcv {

using mgk::cmul;
using mgk::d2_t;
using mgkv::KB;
using mgkv::MAXB;
using mgkv::MAXS;
constexpr int MAXD = 4;        // complex dots per pass (two real scalars each)
constexpr int MAXV = 8;        // vectors per Gram-Schmidt pass

// workgroups of a pass over n complex elements: at least 4 elements per lane, MAXB at most
inline int cxv_grid(long long n) {
  const long long g = (n + (long long)KB * 4 - 1) / ((long long)KB * 4);
  return (int)(g < 1 ? 1 : (g > MAXB ? MAXB : g));
}

// acc[0] + i acc[1] += conj(a) b
__device__ __forceinline__ void cdot_acc(double* acc, d2_t a, d2_t b) {
  acc[0] += a.x * b.x + a.y * b.y;
  acc[1] += a.x * b.y - a.y * b.x;
}
__device__ __forceinline__ void cabs2_acc(double& acc, d2_t a) { acc += a.x * a.x + a.y * a.y; }

// One pass.  Op: NS real scalars (0..MAXS), and at(i, acc): the update of element i.
template <class Op>
__global__ __launch_bounds__(KB) void cxv_pass(const Op op, long long n, double* __restrict__ partial) {
  constexpr int NS = Op::NS;
  double acc[NS > 0 ? NS : 1];
#pragma unroll
  for (int c = 0; c < (NS > 0 ? NS : 1); ++c) acc[c] = 0.0;
  const long long stride = (long long)gridDim.x * KB;
  for (long long i = (long long)blockIdx.x * KB + threadIdx.x; i < n; i += stride) op.at(i, acc);
  if constexpr (NS > 0) {
    __shared__ double red[NS][KB / 64];
#pragma unroll
    for (int c = 0; c < NS; ++c) {
      const double s = mgkv::wave_sum(acc[c]);
      if ((threadIdx.x & 63) == 0) red[c][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x < NS) {
      const double* r = red[threadIdx.x];
      partial[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = (r[0] + r[1]) + (r[2] + r[3]);
    }
  }
}

// ---- the passes.  Bytes per complex element (16-byte values, reads + writes) in the comment of each. ----
// k dots dot(x_c, y_c), c < k <= 4, (re, im) each: 32 k bytes (16 k where x_c == y_c: the second load hits the first's line)
struct OpCDots {
  static constexpr int NS = 2 * MAXD;
  int k;
  const d2_t* x[MAXD];
  const d2_t* y[MAXD];
  __device__ __forceinline__ void at(long long i, double* acc) const {
#pragma unroll
    for (int c = 0; c < MAXD; ++c)
      if (c < k) cdot_acc(acc + 2 * c, x[c][i], y[c][i]);
  }
};
// y = a x (a new basis vector v = w / ||w||; a copy with a = 1): 32 bytes
struct OpCScale {
  static constexpr int NS = 0;
  d2_t a;
  const d2_t* x;
  d2_t* y;
  __device__ __forceinline__ void at(long long i, double*) const { y[i] = cmul(a, x[i]); }
};
// BiCGSTAB: p = r + beta (p - omega v): 64 bytes
struct OpCBicgP {
  static constexpr int NS = 0;
  d2_t beta, omega;
  const d2_t *r, *v;
  d2_t* p;
  __device__ __forceinline__ void at(long long i, double*) const { p[i] = r[i] + cmul(beta, p[i] - cmul(omega, v[i])); }
};
// BiCGSTAB: s = r - alpha v (in r) ; ||s||^2: 48 bytes
struct OpCBicgS {
  static constexpr int NS = 1;
  d2_t alpha;
  const d2_t* v;
  d2_t* r;
  __device__ __forceinline__ void at(long long i, double* acc) const {
    const d2_t s = r[i] - cmul(alpha, v[i]);
    r[i] = s;
    cabs2_acc(acc[0], s);
  }
};
// BiCGSTAB: dot(t, s) (complex), dot(t, t) (real) in one pass over t and s: 32 bytes
struct OpCBicgTS {
  static constexpr int NS = 3;
  const d2_t *t, *s;
  __device__ __forceinline__ void at(long long i, double* acc) const {
    const d2_t tv = t[i];
    cdot_acc(acc, tv, s[i]);
    cabs2_acc(acc[2], tv);
  }
};
// BiCGSTAB: x += alpha phat + omega shat ; r = s - omega t (s held in r) ; ||r||^2 (real), dot(rtld, r) (complex): 128 bytes
struct OpCBicgXR {
  static constexpr int NS = 3;
  d2_t alpha, omega;
  const d2_t *phat, *shat, *t, *rtld;
  d2_t *x, *r;
  __device__ __forceinline__ void at(long long i, double* acc) const {
    x[i] = x[i] + (cmul(alpha, phat[i]) + cmul(omega, shat[i]));
    const d2_t rn = r[i] - cmul(omega, t[i]);
    r[i] = rn;
    cabs2_acc(acc[0], rn);
    cdot_acc(acc + 1, rtld[i], rn);
  }
};
// FGMRES: w -= sum_{j<m} h_j v_j, m <= 8, taken one v_j after the other (the order of the Gram-Schmidt loop) ; ||w||^2:
// 16 (m + 2) bytes.  Also x += Z y (h = -y).
struct OpCGsUpdate {
  static constexpr int NS = 1;
  int m;
  d2_t h[MAXV];
  const d2_t* v[MAXV];
  d2_t* w;
  __device__ __forceinline__ void at(long long i, double* acc) const {
    d2_t wv = w[i];
#pragma unroll
    for (int j = 0; j < MAXV; ++j)
      if (j < m) wv = wv - cmul(h[j], v[j][i]);
    w[i] = wv;
    cabs2_acc(acc[0], wv);
  }
};
// FGMRES, the chained form of modified Gram-Schmidt: the coefficient h_k = *hk is read from HBM (the sum the pass before left
// there), w -= h_k v, and the partials of the NEXT scalar come out of the same pass - dot(u, w) (u = the next basis vector) or,
// with u == nullptr, ||w||^2 in scalar 0 and zero in scalar 1.  48 bytes (64 with u).
struct OpCMgsStep {
  static constexpr int NS = 2;
  const double* hk;
  const d2_t *v, *u;
  d2_t* w;
  __device__ __forceinline__ void at(long long i, double* acc) const {
    const d2_t hv = d2_t{hk[0], hk[1]};
    const d2_t wv = w[i] - cmul(hv, v[i]);
    w[i] = wv;
    if (u) cdot_acc(acc, u[i], wv);
    else cabs2_acc(acc[0], wv);
  }
};

}  // namespace mgcv
