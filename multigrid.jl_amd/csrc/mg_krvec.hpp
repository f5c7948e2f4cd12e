// mg_krvec.hpp - fused vector kernels of the sharded Krylov drivers (mg_dist_krylov.inc): one pass over the vectors of an
// update that also leaves the partial sums of the scalars due at that point of the iteration.
//
// Shape of every kernel (krv_pass<Op>): a grid-stride loop over PAIRS of doubles - one 16-byte load / store per vector,
// lane and trip - with at most one leading and one trailing element handled as scalars, so that vectors whose address is
// 8 bytes past a 16-byte boundary still take the 16-byte path (head = 1).  Vectors of mixed alignment run the scalar path
// for every element (head = n).  Sums: per lane in registers, per wavefront by DPP row operations (no LDS), the 4 wavefronts
// of a workgroup through 32 bytes of LDS per scalar, one partial per workgroup and scalar in HBM (partial[c * gridDim.x +
// block]); krv_final adds them up, one workgroup per scalar.  No floating-point atomics anywhere: the grid is a function of
// n alone, so a rerun adds the same numbers in the same order and gives the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace mgkv {

constexpr int KB = 256;        // threads per workgroup (4 wavefronts of 64)
constexpr int MAXS = 8;        // scalars per pass (and per all-reduce)
constexpr int MAXB = 1024;     // workgroups per pass at most: the partial-sum buffer holds MAXS * MAXB doubles

// workgroups of a pass over n elements: at least 4 pairs per lane, MAXB at most
inline int krv_grid(long long n) {
  const long long g = (n / 2 + (long long)KB * 4 - 1) / ((long long)KB * 4);
  return (int)(g < 1 ? 1 : (g > MAXB ? MAXB : g));
}

// ---- element helpers: the same expression on a double and on a pair ----
__device__ __forceinline__ double kfma(double a, double x, double y) { return fma(a, x, y); }
__device__ __forceinline__ double2 kfma(double a, double2 x, double2 y) { return make_double2(fma(a, x.x, y.x), fma(a, x.y, y.y)); }
__device__ __forceinline__ double kmul(double a, double x) { return a * x; }
__device__ __forceinline__ double2 kmul(double a, double2 x) { return make_double2(a * x.x, a * x.y); }
__device__ __forceinline__ double ksub(double x, double y) { return x - y; }
__device__ __forceinline__ double2 ksub(double2 x, double2 y) { return make_double2(x.x - y.x, x.y - y.y); }
__device__ __forceinline__ double kadd(double x, double y) { return x + y; }
__device__ __forceinline__ double2 kadd(double2 x, double2 y) { return make_double2(x.x + y.x, x.y + y.y); }
__device__ __forceinline__ void kacc(double& acc, double x, double y) { acc = fma(x, y, acc); }
__device__ __forceinline__ void kacc(double& acc, double2 x, double2 y) { acc = fma(x.y, y.y, fma(x.x, y.x, acc)); }
template <class V> __device__ __forceinline__ V kld(const double* p, long long e) { return *reinterpret_cast<const V*>(p + e); }
template <class V> __device__ __forceinline__ void kst(double* p, long long e, V v) { *reinterpret_cast<V*>(p + e) = v; }

// ---- sum over the 64 lanes of a wavefront by DPP: quad swaps, half-row mirror, row mirror leave every lane with the sum of its
//      row of 16; the four row sums are read from lanes 15 / 31 / 47 / 63.  Every lane must be active.
template <int CTRL> __device__ __forceinline__ double dpp_get(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_get(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum(double v) {
  v += dpp_get<0xB1>(v);     // quad_perm [1,0,3,2]
  v += dpp_get<0x4E>(v);     // quad_perm [2,3,0,1]
  v += dpp_get<0x141>(v);    // row_half_mirror
  v += dpp_get<0x140>(v);    // row_mirror
  return (lane_get(v, 15) + lane_get(v, 31)) + (lane_get(v, 47) + lane_get(v, 63));
}

// One pass.  Op: NS scalars (0..MAXS), and at<V>(e, acc): the update of element(s) e (V = double: one, double2: e and e + 1).
template <class Op>
__global__ __launch_bounds__(KB) void krv_pass(const Op op, long long n, long long head, double* __restrict__ partial) {
  constexpr int NS = Op::NS;
  double acc[NS > 0 ? NS : 1];
#pragma unroll
  for (int c = 0; c < (NS > 0 ? NS : 1); ++c) acc[c] = 0.0;
  const long long stride = (long long)gridDim.x * KB, t0 = (long long)blockIdx.x * KB + threadIdx.x;
  const long long n2 = (n - head) >> 1;
  for (long long i = t0; i < n2; i += stride) op.template at<double2>(head + 2 * i, acc);
  const long long nsc = head + ((n - head) & 1);          // scalar elements: [0, head) and the odd one at the end
  for (long long i = t0; i < nsc; i += stride) op.template at<double>(i < head ? i : head + 2 * n2 + (i - head), acc);
  if constexpr (NS > 0) {
    __shared__ double red[NS][KB / 64];
#pragma unroll
    for (int c = 0; c < NS; ++c) {
      const double s = wave_sum(acc[c]);
      if ((threadIdx.x & 63) == 0) red[c][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x < NS) {
      const double* r = red[threadIdx.x];
      partial[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = (r[0] + r[1]) + (r[2] + r[3]);
    }
  }
}
// second pass: out[c] = sum of partial[c * np .. (c + 1) * np), one workgroup per scalar
__global__ __launch_bounds__(KB) void krv_final(const double* __restrict__ partial, int np, double* __restrict__ out) {
  __shared__ double red[KB / 64];
  const double* p = partial + (size_t)blockIdx.x * np;
  double acc = 0.0;
  for (int i = threadIdx.x; i < np; i += KB) acc += p[i];
  const double s = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- the passes.  Bytes per element (8-byte doubles, reads + writes) in the comment of each. ----
// k dots x_c'y_c, c < k <= 8: 16 k bytes (8 k where x_c == y_c: the second load hits the first's line)
struct OpDots {
  static constexpr int NS = MAXS;
  int k;
  const double* x[MAXS];
  const double* y[MAXS];
  template <class V> __device__ __forceinline__ void at(long long e, double* acc) const {
#pragma unroll
    for (int c = 0; c < MAXS; ++c)
      if (c < k) kacc(acc[c], kld<V>(x[c], e), kld<V>(y[c], e));
  }
};
// PCG, behind q = A p: p'q, r'q, q'q in one pass over p, q, r: 24 bytes
struct OpPcgDots {
  static constexpr int NS = 3;
  const double *p, *q, *r;
  template <class V> __device__ __forceinline__ void at(long long e, double* acc) const {
    const V qv = kld<V>(q, e);
    kacc(acc[0], kld<V>(p, e), qv);
    kacc(acc[1], kld<V>(r, e), qv);
    kacc(acc[2], qv, qv);
  }
};
// PCG: x += alpha p ; r -= alpha q ; ||r||^2: 48 bytes
struct OpPcgUpdate {
  static constexpr int NS = 1;
  double alpha;
  const double *p, *q;
  double *x, *r;
  template <class V> __device__ __forceinline__ void at(long long e, double* acc) const {
    kst<V>(x, e, kfma(alpha, kld<V>(p, e), kld<V>(x, e)));
    const V rn = kfma(-alpha, kld<V>(q, e), kld<V>(r, e));
    kst<V>(r, e, rn);
    kacc(acc[0], rn, rn);
  }
};
// y = x + beta y (PCG: p = z + beta p): 24 bytes
struct OpXpby {
  static constexpr int NS = 0;
  double beta;
  const double* x;
  double* y;
  template <class V> __device__ __forceinline__ void at(long long e, double*) const { kst<V>(y, e, kfma(beta, kld<V>(y, e), kld<V>(x, e))); }
};
// y = a x (a new basis vector v = w / ||w||; a copy with a = 1): 16 bytes
struct OpScale {
  static constexpr int NS = 0;
  double a;
  const double* x;
  double* y;
  template <class V> __device__ __forceinline__ void at(long long e, double*) const { kst<V>(y, e, kmul(a, kld<V>(x, e))); }
};
// BiCGSTAB: p = r + beta (p - omega v): 32 bytes
struct OpBicgP {
  static constexpr int NS = 0;
  double beta, omega;
  const double *r, *v;
  double* p;
  template <class V> __device__ __forceinline__ void at(long long e, double*) const {
    kst<V>(p, e, kfma(beta, kfma(-omega, kld<V>(v, e), kld<V>(p, e)), kld<V>(r, e)));
  }
};
// BiCGSTAB: s = r - alpha v (in r) ; ||s||^2: 24 bytes
struct OpBicgS {
  static constexpr int NS = 1;
  double alpha;
  const double* v;
  double* r;
  template <class V> __device__ __forceinline__ void at(long long e, double* acc) const {
    const V s = kfma(-alpha, kld<V>(v, e), kld<V>(r, e));
    kst<V>(r, e, s);
    kacc(acc[0], s, s);
  }
};
// BiCGSTAB: t's, t't in one pass over t and s: 16 bytes
struct OpBicgTS {
  static constexpr int NS = 2;
  const double *t, *s;
  template <class V> __device__ __forceinline__ void at(long long e, double* acc) const {
    const V tv = kld<V>(t, e);
    kacc(acc[0], tv, kld<V>(s, e));
    kacc(acc[1], tv, tv);
  }
};
// BiCGSTAB: x += alpha phat + omega shat ; r = s - omega t (s held in r) ; ||r||^2, rtld'r: 64 bytes
struct OpBicgXR {
  static constexpr int NS = 2;
  double alpha, omega;
  const double *phat, *shat, *t, *rtld;
  double *x, *r;
  template <class V> __device__ __forceinline__ void at(long long e, double* acc) const {
    kst<V>(x, e, kadd(kld<V>(x, e), kfma(omega, kld<V>(shat, e), kmul(alpha, kld<V>(phat, e)))));
    const V rn = kfma(-omega, kld<V>(t, e), kld<V>(r, e));
    kst<V>(r, e, rn);
    kacc(acc[0], rn, rn);
    kacc(acc[1], kld<V>(rtld, e), rn);
  }
};
// FGMRES: w -= sum_{j<m} h_j v_j, m <= 8, taken one v_j after the other (the order of the Gram-Schmidt loop) ; ||w||^2: 8 (m + 2) bytes.
// Also x += Z y (h = -y).
struct OpGsUpdate {
  static constexpr int NS = 1;
  int m;
  double h[MAXS];
  const double* v[MAXS];
  double* w;
  template <class V> __device__ __forceinline__ void at(long long e, double* acc) const {
    V wv = kld<V>(w, e);
#pragma unroll
    for (int j = 0; j < MAXS; ++j)
      if (j < m) wv = kfma(-h[j], kld<V>(v[j], e), wv);
    kst<V>(w, e, wv);
    kacc(acc[0], wv, wv);
  }
};

}  // namespace mgkv
