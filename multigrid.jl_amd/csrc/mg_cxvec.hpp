// mg_cxvec.hpp - fused ComplexF64 vector kernels of the complex Krylov drivers (mg_complex_krylov.inc): one pass over the vectors
// of an update that also leaves the partial sums of the scalars due at that point of the iteration.  The complex counterpart of
// mg_krvec.hpp, whose reduction (mgkv::wave_sum, mgkv::krv_final) and geometry constants it shares.  At the end: the passes of the GMRES
// coarsest solve of a complex hierarchy (cg_mgs_pass, cg_norm_pass, cg_tail, OpCCombine; driven by cx_coarse_gmres, mg_complex.inc).
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
// The combination pass of an FGMRES relaxation on a ComplexF32 hierarchy: x += sum_{j<m} t_j z_j, m <= 8, for complex64 x and z_j
// and double coefficients.  Every element is widened on load, its sum is formed in double in direction order and rounded once on
// the store (the convention of mg_rap_CF32): 8 (m + 2) bytes.
struct OpCRelaxCombineF {
  static constexpr int NS = 0;
  int m;
  d2_t t[MAXV];
  const mgk::f2_t* z[MAXV];
  mgk::f2_t* x;
  __device__ __forceinline__ void at(long long i, double*) const {
    d2_t xv = mgk::cwide(x[i]);
#pragma unroll
    for (int j = 0; j < MAXV; ++j)
      if (j < m) xv = xv + cmul(t[j], mgk::cwide(z[j][i]));
    x[i] = mgk::f2_t{(float)xv.x, (float)xv.y};
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

// x = sum_{j<m} y_j Z_j, m <= CG_M: the combination behind the GMRES coarsest solve (x is written, never read): 16 (m + 1) bytes
constexpr int CG_M = 10;                         // Arnoldi steps of the coarsest solve (MGcycle.jl:160: fgmres(.., 10, maxIter = 1))
constexpr int CG_TAB = (CG_M + 1) * (CG_M + 1);  // its scalar table, see cg_slot
struct OpCCombine {
  static constexpr int NS = 0;
  int m;
  d2_t y[CG_M];
  const d2_t* z[CG_M];
  d2_t* x;
  __device__ __forceinline__ void at(long long i, double*) const {
    d2_t acc = d2_t{0.0, 0.0};
#pragma unroll
    for (int j = 0; j < CG_M; ++j)
      if (j < m) acc = acc + cmul(y[j], z[j][i]);
    x[i] = acc;
  }
};

// ------------------------------------------------------------------------------------------------
// The GMRES coarsest solve of a complex hierarchy (coarseSolveType "GMRES", MGcycle.jl:152-164): one restart of FGMRES(10) from
// x = 0 with the Jacobi preconditioner z = d.*v, enqueued whole and replayed on the host from ONE table of scalars
// (coarse_gmres_replay, mg_krylov_host.hpp).  The table: scalar 0 = ||b||^2; step i from cg_slot(i) = 1 + i^2 + 2 i on: h_0 .. h_i
// (re, im each), then ||w||^2 - (CG_M + 1)^2 doubles.  Step i is w = A z_i with the partials of dot(v_0, w)
// (cx_csr_stream_spmv<CGDOT>), then modified Gram-Schmidt in the reference's order - h_k = dot(v_k, w) conjugating v_k,
// w -= h_k v_k, k ascending - then v_{i+1} = w / ||w|| and z_{i+1} = d.*v_{i+1}.  Two forms of everything behind the product:
//   the chain   cg_mgs_pass x (i + 1), cg_norm_pass: grid-wide passes.  Every pass sums the partials the pass before it left -
//               each workgroup the same numbers in the same order, so all of them hold the same h_k - and workgroup 0 stores
//               the sum into the table: no launch of a final sum between two passes.  i + 3 launches in step i.
//   the tail    cg_tail: ONE workgroup holds w in registers (CG_TAIL_E values per lane), streams v_k from L2 and reduces through
//               DPP and LDS: the whole chain, the norm, the normalisation and z = d.*v in one launch, 2 launches per step; levels of
//               up to CG_TAIL_ROWS rows.
// No atomics; a rerun adds the same numbers in the same order.  ||w|| = 0 (and b = 0) writes zeros, never NaN.
// ------------------------------------------------------------------------------------------------
__host__ __device__ inline int cg_slot(int i) { return 1 + i * i + 2 * i; }
constexpr int CG_TAIL_T = 1024;                       // threads of the one-workgroup tail at most
constexpr int CG_TAIL_E = 8;                          // values of w per lane
constexpr int CG_TAIL_ROWS = CG_TAIL_T * CG_TAIL_E;   // 8192 rows: every geometric coarsest level up to 17^3 = 4913 and beyond

// (sa, sb) = the sums of pa[0 .. np) and pb[0 .. np) in an order fixed by np and KB alone; every lane of the workgroup gets them
__device__ __forceinline__ d2_t cg_sum_partials(const double* __restrict__ pa, const double* __restrict__ pb, int np, double (*red)[KB / 64]) {
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < np; i += KB) {
    a += pa[i];
    if (pb) b += pb[i];
  }
  a = mgkv::wave_sum(a);
  b = mgkv::wave_sum(b);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = a;
    red[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  const d2_t s = d2_t{(red[0][0] + red[0][1]) + (red[0][2] + red[0][3]), (red[1][0] + red[1][1]) + (red[1][2] + red[1][3])};
  __syncthreads();   // (red is written again by the caller's own reduction)
  return s;
}

// one pass of the chain: h_k = the sum of the partials at pprev (re: [0, np), im: [np, 2 np)), stored at tab2 by workgroup 0;
// w -= h_k v; the partials of dot(u, w) (u: the next basis vector) or, with u == nullptr, of ||w||^2 at pout[c * gridDim.x + block]
__global__ __launch_bounds__(KB) void cg_mgs_pass(const double* __restrict__ pprev, int np, double* __restrict__ tab2, const d2_t* __restrict__ v,
                                                  const d2_t* __restrict__ u, d2_t* __restrict__ w, long long n, double* __restrict__ pout) {
  __shared__ double red[2][KB / 64];
  const d2_t hv = cg_sum_partials(pprev, pprev + np, np, red);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    tab2[0] = hv.x;
    tab2[1] = hv.y;
  }
  double acc[2] = {0.0, 0.0};
  const long long stride = (long long)gridDim.x * KB;
  for (long long i = (long long)blockIdx.x * KB + threadIdx.x; i < n; i += stride) {
    const d2_t wv = w[i] - cmul(hv, v[i]);
    w[i] = wv;
    if (u) cdot_acc(acc, u[i], wv);
    else cabs2_acc(acc[0], wv);
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const double s = mgkv::wave_sum(acc[c]);
    if ((threadIdx.x & 63) == 0) red[c][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const double* r = red[threadIdx.x];
    pout[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = (r[0] + r[1]) + (r[2] + r[3]);
  }
}

// the end of a step (and the front, src = b): s2 = the sum of the partials of ||src||^2, stored at tab1 by workgroup 0;
// v = src / sqrt(s2) (zeros where s2 == 0; v may be src itself) and z = d.*v (z == nullptr: the last step has no next direction)
__global__ __launch_bounds__(KB) void cg_norm_pass(const double* __restrict__ pprev, int np, double* __restrict__ tab1, const d2_t* src, d2_t* v,
                                                   const d2_t* __restrict__ d, d2_t* __restrict__ z, long long n) {
  __shared__ double red[2][KB / 64];
  const double s2 = cg_sum_partials(pprev, nullptr, np, red).x;
  if (blockIdx.x == 0 && threadIdx.x == 0) tab1[0] = s2;
  const double nrm = sqrt(s2);
  const long long stride = (long long)gridDim.x * KB;
  for (long long i = (long long)blockIdx.x * KB + threadIdx.x; i < n; i += stride) {
    const d2_t a = src[i];
    const d2_t o = nrm > 0.0 ? d2_t{a.x / nrm, a.y / nrm} : d2_t{0.0, 0.0};
    v[i] = o;
    if (z) z[i] = cmul(d[i], o);
  }
}

// The one-workgroup form of everything behind the product of a step (nk = i + 1 basis vectors V_0 .. V_i, columns ld apart, w = src
// = vout = V_{i+1}), and of the front (nk = 0, src = b, vout = V_0).  tab: the step's slot (h_k at tab[2 k], ||w||^2 at tab[2 nk]).
// h_0 comes from the product's partials (pprev: re [0, np), im [np, 2 np)); h_k, k >= 1, from the block reduction of dot(v_k, w).
// blockDim.x: a multiple of 64 with blockDim.x * CG_TAIL_E >= n.  The reductions alternate between two LDS slots, one barrier each.
__global__ __launch_bounds__(CG_TAIL_T) void cg_tail(const double* __restrict__ pprev, int np, int nk, double* __restrict__ tab,
                                                     const d2_t* __restrict__ Vb, long long ld, const d2_t* src, d2_t* vout,
                                                     const d2_t* __restrict__ d, d2_t* __restrict__ z, int n) {
  __shared__ double red[2][2][CG_TAIL_T / 64];
  const int tid = threadIdx.x, T = blockDim.x, nw = T >> 6;
  int par = 0;
  auto block_sum2 = [&](double a, double b) -> d2_t {
    a = mgkv::wave_sum(a);
    b = mgkv::wave_sum(b);
    if ((tid & 63) == 0) {
      red[par][0][tid >> 6] = a;
      red[par][1][tid >> 6] = b;
    }
    __syncthreads();
    double sa = 0.0, sb = 0.0;
    for (int q = 0; q < nw; ++q) {   // every lane the same order
      sa += red[par][0][q];
      sb += red[par][1][q];
    }
    par ^= 1;
    return d2_t{sa, sb};
  };
  d2_t w[CG_TAIL_E];
#pragma unroll
  for (int e = 0; e < CG_TAIL_E; ++e) {
    const int i = tid + e * T;
    w[e] = i < n ? src[i] : d2_t{0.0, 0.0};
  }
  for (int k = 0; k < nk; ++k) {
    const d2_t* __restrict__ vk = Vb + (size_t)k * (size_t)ld;
    d2_t vv[CG_TAIL_E];
#pragma unroll
    for (int e = 0; e < CG_TAIL_E; ++e) {
      const int i = tid + e * T;
      vv[e] = i < n ? vk[i] : d2_t{0.0, 0.0};
    }
    double acc[2] = {0.0, 0.0};
    if (k == 0) {
      for (int i = tid; i < np; i += T) {
        acc[0] += pprev[i];
        acc[1] += pprev[np + i];
      }
    } else {
#pragma unroll
      for (int e = 0; e < CG_TAIL_E; ++e) cdot_acc(acc, vv[e], w[e]);
    }
    const d2_t hv = block_sum2(acc[0], acc[1]);
    if (tid == 0) {
      tab[2 * k] = hv.x;
      tab[2 * k + 1] = hv.y;
    }
#pragma unroll
    for (int e = 0; e < CG_TAIL_E; ++e) w[e] = w[e] - cmul(hv, vv[e]);
  }
  double sq = 0.0;
#pragma unroll
  for (int e = 0; e < CG_TAIL_E; ++e) cabs2_acc(sq, w[e]);
  const double s2 = block_sum2(sq, 0.0).x;
  if (tid == 0) tab[2 * nk] = s2;
  const double nrm = sqrt(s2);
#pragma unroll
  for (int e = 0; e < CG_TAIL_E; ++e) {
    const int i = tid + e * T;
    if (i < n) {
      const d2_t o = nrm > 0.0 ? d2_t{w[e].x / nrm, w[e].y / nrm} : d2_t{0.0, 0.0};
      vout[i] = o;
      if (z) z[i] = cmul(d[i], o);
    }
  }
}

}  // namespace mgcv
