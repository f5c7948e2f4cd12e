// mg_dense_inv.hpp - gfx950 kernels of the dense inverse with partial pivoting (the coarsest solve's explicit inverse, built in HBM).
//
// One template, two instantiations: double and d2_t (interleaved (re, im), as cx_dense_matvec reads it).
//
// Algorithm: blocked in-place Gauss-Jordan with row interchanges, panels of DI_NB = 64 columns ("Dense inverse on the
// device").  The work matrix W is ld x ld row-major, ld = n rounded up to a multiple of 64, the padding zero.  Per panel J = [k0, k0+64):
//   di_strip_load   S <- W[:, J] (n x 64, row-major), stage 1 of the pivot search of column k0
//   di_step         one launch per column k: stage 2 of the pivot search (every workgroup reduces the same partials in the same
//                   order), the interchange, the scaled pivot row, the rank-1 update of the whole strip, stage 1 of column k+1.
//                   Reads one strip and one set of partials, writes the other pair: no workgroup reads what another one writes.
//   di_swap_rows    the panel's interchanges on every column outside J, then R <- W[J, :]
//   di_strip_store  W[:, J] <- S, and S transposed (64 x ld) for the update
//   di_update       W[i, j] = (i in J ? 0 : W[i, j]) + sum_k S[i, k] R[k, j], j outside J: the LDS-tiled FP64 GEMM, rank 64
// After the last panel: di_perm turns the recorded pivots into the column permutation (the interchanges undone from the last to the
// first), di_gather writes the inverse row-major n x n.  Every stage is a launch of its own; the pivots and the singular flag stay in
// device memory; no atomics, no barrier between workgroups.  Pivot of column k: the largest |re| + |im| among rows k .. n-1, ties to
// the lowest row; a zero or non-finite pivot stores k + 1 in flag[0] (the first such column wins).
#pragma once
#include "mg_complex.hpp"

namespace mgk {

constexpr int DI_NB = 64;     // panel width = tile of the update
constexpr int DI_KC = 32;     // columns of the panel staged in LDS at a time
constexpr int DI_ROWS = 16;   // strip rows per workgroup (4 per wavefront, one lane per strip column)

__device__ __forceinline__ double di_cabs1(double a) { return fabs(a); }
__device__ __forceinline__ double di_cabs1(d2_t a) { return fabs(a.x) + fabs(a.y); }
__device__ __forceinline__ double di_mul(double a, double b) { return a * b; }
__device__ __forceinline__ d2_t di_mul(d2_t a, d2_t b) { return cmul(a, b); }
__device__ __forceinline__ double di_recip(double a) { return 1.0 / a; }
__device__ __forceinline__ d2_t di_recip(d2_t a) {
  const double s = a.x * a.x + a.y * a.y;
  return d2_t{a.x / s, -a.y / s};
}
__device__ __forceinline__ void di_fma(double& c, double a, double b) { c = fma(a, b, c); }
__device__ __forceinline__ void di_fma(d2_t& c, d2_t a, d2_t b) {
  c.x = fma(a.x, b.x, c.x);
  c.x = fma(-a.y, b.y, c.x);
  c.y = fma(a.x, b.y, c.y);
  c.y = fma(a.y, b.x, c.y);
}
template <typename T> __device__ __forceinline__ T di_zero();
template <> __device__ __forceinline__ double di_zero<double>() { return 0.0; }
template <> __device__ __forceinline__ d2_t di_zero<d2_t>() { return d2_t{0.0, 0.0}; }
// the key of the pivot search: non-finite entries rank above every finite one, so that they are chosen and flagged at once
template <typename T>
__device__ __forceinline__ double di_key(T a) {
  const double v = di_cabs1(a);
  return isfinite(v) ? v : INFINITY;
}
__device__ __forceinline__ bool di_better(double v, int i, double bv, int bi) { return v > bv || (v == bv && i < bi); }

// stage 1 of the pivot search in a workgroup: cand[DI_ROWS] holds the keys of its rows (-1: not eligible), first row `r0`
__device__ __forceinline__ void di_stage1(const double* cand, int r0, double* pv, int* pi) {
  double bv = -1.0;
  int bi = INT_MAX;
  for (int q = 0; q < DI_ROWS; ++q)
    if (cand[q] >= 0.0 && di_better(cand[q], r0 + q, bv, bi)) {
      bv = cand[q];
      bi = r0 + q;
    }
  pv[blockIdx.x] = bv;
  pi[blockIdx.x] = bi;
}

// W <- the CSR operator (one thread per row; entries of one row are added in stored order).  VT: the stored values (double, d2_t, or
// the float pairs of a ComplexF32 handle, widened here).
__device__ __forceinline__ double di_widen(double v, double*) { return v; }
__device__ __forceinline__ d2_t di_widen(d2_t v, d2_t*) { return v; }
__device__ __forceinline__ d2_t di_widen(f2_t v, d2_t*) { return d2_t{(double)v.x, (double)v.y}; }
template <typename T, typename VT>
__global__ __launch_bounds__(BLK) void di_scatter(const int* __restrict__ rowptr, const int* __restrict__ colidx, const VT* __restrict__ val,
                                                  int n, int ld, T* __restrict__ W) {
  const int r = blockIdx.x * BLK + threadIdx.x;
  if (r >= n) return;
  for (int e = rowptr[r]; e < rowptr[r + 1]; ++e) {
    const int c = colidx[e];
    if (c >= 0 && c < n) W[(size_t)r * ld + c] += di_widen(val[e], (T*)nullptr);
  }
}

// W (ld x ld, row-major) <- a column-major n x n matrix, and back
template <typename T>
__global__ __launch_bounds__(BLK) void di_from_colmajor(const T* __restrict__ A, int n, int ld, T* __restrict__ W) {
  const size_t e = (size_t)blockIdx.x * BLK + threadIdx.x;
  if (e >= (size_t)n * n) return;
  const int i = (int)(e % n), j = (int)(e / n);
  W[(size_t)i * ld + j] = A[e];
}
template <typename T>
__global__ __launch_bounds__(BLK) void di_to_colmajor(const T* __restrict__ X, int n, T* __restrict__ out) {
  const size_t e = (size_t)blockIdx.x * BLK + threadIdx.x;
  if (e >= (size_t)n * n) return;
  const int i = (int)(e % n), j = (int)(e / n);
  out[e] = X[(size_t)i * n + j];
}

template <typename T>
__global__ __launch_bounds__(256) void di_strip_load(const T* __restrict__ W, int ld, int n, int k0, T* __restrict__ S,
                                                     double* __restrict__ pv, int* __restrict__ pi) {
  __shared__ double cand[DI_ROWS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r0 = blockIdx.x * DI_ROWS;
  for (int q = 0; q < 4; ++q) {
    const int r = r0 + w * 4 + q;
    if (r < n) {
      const T v = W[(size_t)r * ld + k0 + lane];
      S[(size_t)r * DI_NB + lane] = v;
      if (lane == 0) cand[w * 4 + q] = r >= k0 ? di_key(v) : -1.0;
    } else if (lane == 0) {
      cand[w * 4 + q] = -1.0;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) di_stage1(cand, r0, pv, pi);
}

template <typename T>
__global__ __launch_bounds__(256) void di_step(const T* __restrict__ Sin, T* __restrict__ Sout, int n, int k0, int kk,
                                               const double* __restrict__ pv_in, const int* __restrict__ pi_in, double* __restrict__ pv_out,
                                               int* __restrict__ pi_out, int nblk, int* __restrict__ ipiv, int* __restrict__ flag) {
  __shared__ double sv[256];
  __shared__ int si[256];
  __shared__ double cand[DI_ROWS];
  const int tid = threadIdx.x, k = k0 + kk;
  // stage 2: the same partials in the same order in every workgroup
  double bv = -1.0;
  int bi = INT_MAX;
  for (int b = tid; b < nblk; b += 256) {
    const double v = pv_in[b];
    const int i = pi_in[b];
    if (di_better(v, i, bv, bi)) { bv = v; bi = i; }
  }
  sv[tid] = bv;
  si[tid] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s && di_better(sv[tid + s], si[tid + s], sv[tid], si[tid])) {
      sv[tid] = sv[tid + s];
      si[tid] = si[tid + s];
    }
    __syncthreads();
  }
  const int p = (si[0] >= k && si[0] < n) ? si[0] : k;   // (in range whatever the values are)
  const int lane = tid & 63, w = tid >> 6, r0 = blockIdx.x * DI_ROWS;
  const T piv = Sin[(size_t)p * DI_NB + kk];
  const T rinv = di_recip(piv);
  if (blockIdx.x == 0 && tid == 0) {
    ipiv[k] = p;
    const double a = di_cabs1(piv);
    if (!(isfinite(a) && a > 0.0) && flag[0] == 0) flag[0] = k + 1;
  }
  T srow = di_mul(Sin[(size_t)p * DI_NB + lane], rinv);   // the pivot row, scaled; its own column holds 1 / pivot
  if (lane == kk) srow = rinv;
  for (int q = 0; q < 4; ++q) {
    const int r = r0 + w * 4 + q;
    double key = -1.0;
    if (r < n) {
      T o = srow;
      if (r != k) {
        const size_t src = (size_t)(r == p ? k : r) * DI_NB;
        const T v = Sin[src + lane], f = Sin[src + kk];
        o = lane == kk ? di_zero<T>() - di_mul(f, rinv) : v - di_mul(f, srow);
      }
      Sout[(size_t)r * DI_NB + lane] = o;
      if (r > k) key = di_key(o);
    }
    if (kk + 1 < DI_NB && lane == kk + 1) cand[w * 4 + q] = key;
  }
  if (kk + 1 >= DI_NB) return;
  __syncthreads();
  if (tid == 0) di_stage1(cand, r0, pv_out, pi_out);
}

// the panel's interchanges on the columns outside it (one thread per column), then R <- W[k0 .. k0+63, :]
template <typename T>
__global__ __launch_bounds__(BLK) void di_swap_rows(T* __restrict__ W, int ld, int k0, int nbw, const int* __restrict__ ipiv, T* __restrict__ R) {
  const int j = blockIdx.x * BLK + threadIdx.x;
  if (j >= ld || (j >= k0 && j < k0 + DI_NB)) return;
  for (int kk = 0; kk < nbw; ++kk) {
    const int k = k0 + kk, p = ipiv[k];
    if (p != k) {
      const T a = W[(size_t)k * ld + j], b = W[(size_t)p * ld + j];
      W[(size_t)k * ld + j] = b;
      W[(size_t)p * ld + j] = a;
    }
  }
  for (int kk = 0; kk < DI_NB; ++kk) R[(size_t)kk * ld + j] = W[(size_t)(k0 + kk) * ld + j];
}

// W[:, J] <- S and St <- S' (64 x ld); rows n .. ld-1 of S are zero
template <typename T>
__global__ __launch_bounds__(256) void di_strip_store(const T* __restrict__ S, T* __restrict__ W, T* __restrict__ St, int ld, int k0) {
  __shared__ T tile[DI_ROWS][DI_NB + 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r0 = blockIdx.x * DI_ROWS;
  for (int q = 0; q < 4; ++q) {
    const int r = r0 + w * 4 + q;   // (ld is a multiple of 64: r < ld)
    const T v = S[(size_t)r * DI_NB + lane];
    W[(size_t)r * ld + k0 + lane] = v;
    tile[w * 4 + q][lane] = v;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < DI_ROWS * DI_NB; e += 256) {
    const int c = e / DI_ROWS, q = e % DI_ROWS;
    St[(size_t)c * ld + r0 + q] = tile[q][c];
  }
}

// the update: a 64 x 64 tile of W per workgroup, 4 x 4 values per thread, the panel staged in LDS 32 columns at a time
template <typename T>
__global__ __launch_bounds__(256) void di_update(T* __restrict__ W, int ld, const T* __restrict__ St, const T* __restrict__ R, int k0) {
  const int j0 = blockIdx.x * DI_NB, i0 = blockIdx.y * DI_NB;
  if (j0 == k0) return;
  __shared__ T As[DI_KC][DI_NB];
  __shared__ T Bs[DI_KC][DI_NB];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  T acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = di_zero<T>();
  for (int kc = 0; kc < DI_NB; kc += DI_KC) {
    for (int e = tid; e < DI_KC * DI_NB; e += 256) {
      const int kk = e >> 6, c = e & 63;
      As[kk][c] = St[(size_t)(kc + kk) * ld + i0 + c];
      Bs[kk][c] = R[(size_t)(kc + kk) * ld + j0 + c];
    }
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < DI_KC; ++kk) {
      T a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = As[kk][ty * 4 + r];
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = Bs[kk][tx + 16 * c];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) di_fma(acc[r][c], a[r], b[c]);
    }
    __syncthreads();
  }
  const bool add = i0 != k0;   // the panel's own rows: D^-1 times the old rows, nothing added
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const size_t idx = (size_t)(i0 + ty * 4 + r) * ld + j0 + tx + 16 * c;
      W[idx] = add ? W[idx] + acc[r][c] : acc[r][c];
    }
}

// src[j]: the column of W that becomes column j of the inverse (the interchanges undone as column swaps, last first)
// (one workgroup, the chain of swaps by one thread in LDS: n <= DI_MAX)
constexpr int DI_MAX = 8192;
__global__ __launch_bounds__(BLK) void di_perm(const int* __restrict__ ipiv, int n, int* __restrict__ src) {
  __shared__ int s[DI_MAX];
  __shared__ int pv[DI_MAX];
  for (int j = threadIdx.x; j < n; j += BLK) {
    s[j] = j;
    pv[j] = ipiv[j];
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = n - 1; k >= 0; --k) {
      const int p = pv[k];
      if (p != k && p >= 0 && p < n) {
        const int t = s[k];
        s[k] = s[p];
        s[p] = t;
      }
    }
  __syncthreads();
  for (int j = threadIdx.x; j < n; j += BLK) src[j] = s[j];
}

template <typename T>
__global__ __launch_bounds__(BLK) void di_gather(const T* __restrict__ W, int ld, int n, const int* __restrict__ src, T* __restrict__ out) {
  const int j = blockIdx.x * BLK + threadIdx.x, i = blockIdx.y;
  if (j < n) out[(size_t)i * n + j] = W[(size_t)i * ld + src[j]];
}

}  // namespace mgk
