// mg_cxblk_coarse.hpp - the passes of the block GMRES coarsest solve of a complex hierarchy (coarseSolveType "GMRES" given a block of
// right-hand sides, MGcycle.jl:165-167: blockFGMRES(A_c, B, 10, tol = 0.01, maxIter = 1, M = d.*, X = 0)); driven by
// cx_coarse_block_gmres (mg_complex.inc), the block counterpart of the single-vector passes at the end of mg_cxvec.hpp.
//
// Blocks are row-major [n][k] ComplexF64, 1 <= k <= BLK_KMAX.  One restart is enqueued whole: V_0, xi_0 = cholqr2(B); in step j
// Z_j = d.*V_j, W = A_c Z_j (cx_csr_stream_spmm), block modified Gram-Schmidt in ascending order - H_ij = V_i^H W, W -= V_i H_ij - and
// V_{j+1}, H_{j+1,j} = cholqr2(W): Cholesky QR applied twice, R = R2 R1, with the semidefinite factor of sm_chol_semidefinite (real
// pivots; a column with g <= 0 or d <= 1e-14 g is dropped: a zero row of R, a zero column of Q).
//
// Everything behind the product is a chain of grid-wide launches of ONE kernel, cb_pass:
//   1. every workgroup sums the k x k partials the launch before it left ([np][k*k], cx_blk_gram_onepass's layout): lane group g adds
//      the partials g, g + groups, ... and the groups are added in group order - all workgroups the same numbers in the same order,
//      so all of them hold the same matrix.  No launch exists only to sum.
//   2. the small algebra, redundantly per workgroup, in LDS: nothing for a Gram-Schmidt pass (the sum IS H_ij); for a Cholesky pass
//      the factor R (one barrier per column) and its triangular pseudo-inverse T (one lane per row of T, no barrier).
//   3. the update of the workgroup's tiles - W -= V_i H_ij, or Q = W T - one lane per entry, the tile rows staged in LDS by coalesced
//      16-byte loads (a tile is GRAM_TILE / kk rows, kk = pow2 >= k: cx_blk_gram_onepass's tiles), and from the rows just written the
//      partials of the next Gram matrix (V_{i+1}^H W, W^H W after the last Gram-Schmidt pass, Q^H Q after the first Cholesky pass) by
//      cx_gram_tile's lane layout.  The second Cholesky pass also writes Z_{j+1} = d.*V_{j+1} and leaves no partials.
//   4. workgroup 0 stores H_ij / R1 / R2 R1 (and ||B||_F^2 = trace(B^H B) in the front) into the device table.
// No atomics; the grid is a function of n and k alone: a rerun gives the same bits.  B = 0, W = 0 and a zero column give zeros (a
// dropped pivot is never divided by), never NaN.
//
// Bytes per pass over a block of n k values (16 bytes each): Gram-Schmidt 4 n k (W read + written, V_i, V_{i+1}; 3 n k for the last),
// first Cholesky 2 n k, second 3 n k (2 n k without Z); the k x k partials are np * 16 k^2 bytes read by every workgroup from L2.
#pragma once
#include "mg_complex.hpp"

namespace mgcb {

using mgk::BLK;
using mgk::BLK_KMAX;
using mgk::cmul;
using mgk::d2_t;
using mgk::GRAM_TILE;
using mgk::GramLane;

constexpr int CB_M = 10;          // block Arnoldi steps (MGcycle.jl:166: blockFGMRES(.., 10, maxIter = 1))
constexpr int CB_MAXWG = 256;     // workgroups of a pass at most: one per CU
constexpr int CB_MAXPART = 1024;  // ... and at most this many / kk of them (kk = pow2 >= k): EVERY workgroup reads all np partials of
                                  // 16 k^2 bytes, np^2 k^2 16 bytes per pass from L2 - 256 MB at k = 16 with 256 workgroups, 17 MB with
                                  // 64.  A bound on that traffic, not a measured gain: at 35 937 rows x 16 the solve took 8.70 ms with
                                  // 256 workgroups and 8.66 ms with 64 (profiles/complex_block_coarse_gmres.md)
constexpr int CB_MGS = 0, CB_CHOL = 1;
constexpr int CB_KK = BLK_KMAX * BLK_KMAX;

// workgroups of a pass: one per tile, min(CB_MAXWG, CB_MAXPART / kk) at most
inline int cb_grid(long long n, int lgk) {
  const long long tr = GRAM_TILE >> lgk;
  const long long g = (n + tr - 1) / tr;
  const long long cap = (CB_MAXPART >> lgk) < CB_MAXWG ? (CB_MAXPART >> lgk) : CB_MAXWG;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

struct CbPass {
  const d2_t* pprev;   // the partials of this pass's matrix: [np][k*k]
  int np;
  int k, lgk;
  long long n;
  const d2_t* src;     // CHOL: the block that is scaled (may be W itself)
  d2_t* W;             // MGS: updated in place; CHOL: Q
  const d2_t* V;       // MGS: V_i
  const d2_t* U;       // MGS: V_{i+1}, or nullptr after the last one (the partials are those of W^H W)
  const d2_t* d;       // CHOL, with Z: the Jacobi vector
  d2_t* Z;             // CHOL: Z = d.*Q (nullptr: none)
  d2_t* out;           // workgroup 0: H_ij (MGS), R (CHOL without r1), R2 R1 (CHOL with r1), k x k row-major
  const d2_t* r1;      // CHOL, second pass: R1 as the first pass stored it
  double* trace;       // CHOL: trace of the Gram matrix (nullptr: none)
  d2_t* pout;          // the partials of the next Gram matrix: [gridDim.x][k*k] (nullptr: none)
};

// sS (k x k, row-major) = the sum of the np partials; red: BLK values of scratch
__device__ __forceinline__ void cb_sum_partials(const d2_t* pprev, int np, int k, const GramLane& L, d2_t* red, d2_t* sS) {
  d2_t t = d2_t{0.0, 0.0};
  if (L.on)
    for (int p = L.g; p < np; p += L.groups) t += pprev[(size_t)p * k * k + L.a * k + L.b];
  red[threadIdx.x] = t;
  __syncthreads();
  if (L.g == 0 && L.on) {
    const int kk2 = BLK / L.groups;
    d2_t s = d2_t{0.0, 0.0};
    for (int g = 0; g < L.groups; ++g) s += red[g * kk2 + threadIdx.x];
    sS[L.a * k + L.b] = s;
  }
  __syncthreads();
}

// sR = the upper triangular semidefinite Cholesky factor of the Hermitian sG, sT = its triangular pseudo-inverse (W T = W R^+)
__device__ __forceinline__ void cb_chol_pinv(const d2_t* sG, d2_t* sR, d2_t* sT, int k) {
  const int j = threadIdx.x;
  for (int t = j; t < k * k; t += BLK) {
    sR[t] = d2_t{0.0, 0.0};
    sT[t] = d2_t{0.0, 0.0};
  }
  __syncthreads();
  for (int c = 0; c < k; ++c) {
    if (j >= c && j < k) {   // row c of R, one lane per column; every lane forms the pivot from the same numbers
      const double g = sG[c * k + c].x;
      double s = 0.0;
      for (int a = 0; a < c; ++a) s += mgk::cabs2(sR[a * k + c]);
      const double dd = g - s;
      if (!(g <= 0.0 || dd <= 1e-14 * g)) {
        const double rc = sqrt(dd);
        if (j == c) {
          sR[c * k + c] = d2_t{rc, 0.0};
        } else {
          d2_t t = sG[c * k + j];
          for (int a = 0; a < c; ++a) {
            const d2_t ra = sR[a * k + c];
            t = t - cmul(d2_t{ra.x, -ra.y}, sR[a * k + j]);
          }
          sR[c * k + j] = d2_t{t.x / rc, t.y / rc};
        }
      }
    }
    __syncthreads();
  }
  if (j < k) {   // row j of T: T[j][c] = ((j == c) - sum_{a < c} T[j][a] R[a][c]) / R[c][c], zero for a dropped pivot
    for (int c = j; c < k; ++c) {
      const double rc = sR[c * k + c].x;
      if (rc == 0.0) continue;
      d2_t t = d2_t{j == c ? 1.0 : 0.0, 0.0};
      for (int a = j; a < c; ++a) t = t - cmul(sT[j * k + a], sR[a * k + c]);
      sT[j * k + c] = d2_t{t.x / rc, t.y / rc};
    }
  }
  __syncthreads();
}

// the LDS of a pass: three tiles, the reduction scratch, the summed matrix (56 KiB)
struct CbLds {
  d2_t *sIn, *sOut, *sX, *red, *sS;
};
#define CB_LDS(name)                                                                          \
  __shared__ d2_t name##_in[GRAM_TILE], name##_out[GRAM_TILE], name##_x[GRAM_TILE], name##_red[BLK], name##_s[CB_KK]; \
  const CbLds name = {name##_in, name##_out, name##_x, name##_red, name##_s}

// one pass by the workgroups of the grid it is called from (blockIdx.x of gridDim.x; the one-workgroup form calls it with a grid of 1)
template <int MODE>
__device__ __forceinline__ void cb_pass_body(const CbPass& p, const CbLds& lds) {
  d2_t *sIn = lds.sIn, *sOut = lds.sOut, *sX = lds.sX, *red = lds.red, *sS = lds.sS;
  constexpr int PER = GRAM_TILE / BLK;
  static_assert(2 * CB_KK <= GRAM_TILE, "R and T of a Cholesky pass live in the tile a Gram-Schmidt pass stages V_{i+1} in");
  const int tid = threadIdx.x, k = p.k;
  const GramLane L(k, p.lgk);
  cb_sum_partials(p.pprev, p.np, k, L, red, sS);
  d2_t* sT = sX + CB_KK;   // (CHOL: sR = sX)
  if (MODE == CB_CHOL) {
    cb_chol_pinv(sS, sX, sT, k);
    if (blockIdx.x == 0) {
      if (p.trace && tid == 0) {
        double s = 0.0;
        for (int c = 0; c < k; ++c) s += sS[c * k + c].x;
        p.trace[0] = s;
      }
      if (tid < k * k) {
        const int a = tid / k, b = tid - a * k;
        d2_t o = sX[tid];
        if (p.r1) {   // R2 R1, both upper triangular
          o = d2_t{0.0, 0.0};
          for (int c = a; c <= b; ++c) o += cmul(sX[a * k + c], p.r1[c * k + b]);
        }
        p.out[tid] = o;
      }
    }
  } else if (blockIdx.x == 0 && tid < k * k) {
    p.out[tid] = sS[tid];
  }
  const int tr = GRAM_TILE >> p.lgk;                // rows of a tile
  const int tlen = tr * k;                          // its entries (<= GRAM_TILE)
  const long long ntiles = (p.n + tr - 1) / tr, total = p.n * k;
  const bool cross = MODE == CB_MGS && p.U != nullptr;
  d2_t acc = d2_t{0.0, 0.0};
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {   // (uniform over the workgroup)
    const long long base = tile * tlen;
    const int here = (int)((total - base) < (long long)tlen ? (total - base) : (long long)tlen);
    d2_t wreg[PER];
#pragma unroll
    for (int it = 0; it < PER; ++it) {
      const int l = it * BLK + tid;
      wreg[it] = d2_t{0.0, 0.0};
      if (l < here) {
        if (MODE == CB_MGS) {
          sIn[l] = p.V[base + l];
          if (cross) sX[l] = p.U[base + l];
          wreg[it] = p.W[base + l];
        } else {
          sIn[l] = p.src[base + l];
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < PER; ++it) {
      const int l = it * BLK + tid;
      if (l < here) {
        const int r = l / k, b = l - r * k;
        const d2_t* row = sIn + r * k;
        d2_t o;
        if (MODE == CB_MGS) {
          o = wreg[it];
          for (int a = 0; a < k; ++a) o = o - cmul(row[a], sS[a * k + b]);
        } else {
          o = d2_t{0.0, 0.0};
          for (int a = 0; a <= b; ++a) o += cmul(row[a], sT[a * k + b]);
        }
        p.W[base + l] = o;
        sOut[l] = o;
        if (MODE == CB_CHOL && p.Z) p.Z[base + l] = cmul(p.d[tile * tr + r], o);
      }
    }
    if (p.pout) {
      __syncthreads();
      mgk::cx_gram_tile(cross ? sX : sOut, sOut, here / k, k, L, acc);
    }
    __syncthreads();
  }
  if (p.pout) mgk::cx_gram_store(red, acc, k, L, p.pout);
}

template <int MODE>
__global__ __launch_bounds__(BLK) void cb_pass(const CbPass p) {
  CB_LDS(lds);
  cb_pass_body<MODE>(p, lds);
}

// ---- the one-workgroup form of everything behind the product of a step (and of the front): the Gram matrix V_0^H W, the nk = j + 1
// Gram-Schmidt passes and the two Cholesky passes run one after the other in ONE launch of ONE workgroup - the same code as the chain,
// called with a grid of 1, a barrier between the passes, the k x k partials handed on through 2 x k^2 values of HBM scratch.  W and
// the V_i stream through L2 (a level this form serves holds at most CB_TAIL_ENTRIES values per block).  2 launches per step, 1 for
// the front.  The sums are added in another order than the chain's (one workgroup walks all tiles), each in a fixed one.
constexpr int CB_TAIL_ENTRIES = 8192;      // n_c * k at most (mgcv::CG_TAIL_ROWS)
struct CbTail {
  int k, lgk, nk;      // nk: basis blocks to orthogonalise against (0: the front)
  long long n, ld;     // rows; entries between two basis blocks
  const d2_t* V;       // V_0 (nk > 0)
  const d2_t* src;     // the block cholqr2 scales: W itself, or B in the front
  d2_t* W;             // V_{nk}
  const d2_t* d;
  d2_t* Z;             // Z_{nk} = d.*V_{nk} (nullptr: none)
  d2_t* slot;          // the step's blocks of the table: H_0 .. H_{nk-1}, then R2 R1
  d2_t* r1;
  double* trace;       // front: ||B||_F^2
  d2_t* part;          // 2 x k*k values of scratch
};
// the partials of X^H Y over all tiles of this workgroup's share (X == Y: loaded once)
__device__ __forceinline__ void cb_gram_body(const d2_t* X, const d2_t* Y, long long n, int k, int lgk, const CbLds& lds, d2_t* pout) {
  constexpr int PER = GRAM_TILE / BLK;
  const int tid = threadIdx.x;
  const GramLane L(k, lgk);
  const bool same = X == Y;
  const int tr = GRAM_TILE >> lgk, tlen = tr * k;
  const long long ntiles = (n + tr - 1) / tr, total = n * k;
  d2_t acc = d2_t{0.0, 0.0};
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long base = tile * tlen;
    const int here = (int)((total - base) < (long long)tlen ? (total - base) : (long long)tlen);
#pragma unroll
    for (int it = 0; it < PER; ++it) {
      const int l = it * BLK + tid;
      if (l < here) {
        lds.sIn[l] = X[base + l];
        if (!same) lds.sOut[l] = Y[base + l];
      }
    }
    __syncthreads();
    mgk::cx_gram_tile(lds.sIn, same ? lds.sIn : lds.sOut, here / k, k, L, acc);
    __syncthreads();
  }
  mgk::cx_gram_store(lds.red, acc, k, L, pout);
}
__global__ __launch_bounds__(BLK) void cb_tail(const CbTail t) {
  CB_LDS(lds);
  const size_t kk = (size_t)t.k * t.k;
  d2_t* part[2] = {t.part, t.part + kk};
  CbPass p = {};
  p.np = 1; p.k = t.k; p.lgk = t.lgk; p.n = t.n; p.d = t.d; p.W = t.W;
  if (t.nk > 0) cb_gram_body(t.V, t.W, t.n, t.k, t.lgk, lds, part[0]);
  else cb_gram_body(t.src, t.src, t.n, t.k, t.lgk, lds, part[0]);
  __syncthreads();
  int cur = 0;
  for (int i = 0; i < t.nk; ++i) {
    p.pprev = part[cur]; p.V = t.V + (size_t)i * (size_t)t.ld; p.U = i + 1 < t.nk ? t.V + (size_t)(i + 1) * (size_t)t.ld : nullptr;
    p.out = t.slot + (size_t)i * kk; p.pout = part[1 - cur];
    cb_pass_body<CB_MGS>(p, lds);
    __syncthreads();
    cur = 1 - cur;
  }
  p.V = p.U = nullptr;
  p.pprev = part[cur]; p.src = t.src; p.out = t.r1; p.trace = t.trace; p.pout = part[1 - cur];
  cb_pass_body<CB_CHOL>(p, lds);
  __syncthreads();
  p.pprev = part[1 - cur]; p.src = t.W; p.out = t.slot + (size_t)t.nk * kk; p.r1 = t.r1; p.trace = nullptr; p.pout = nullptr; p.Z = t.Z;
  cb_pass_body<CB_CHOL>(p, lds);
}

// X = sum_{j < used} Z_j Y_j: Z_j row-major blocks ldz entries apart, Y the (used k) x k solution of the block least squares, row-major
// (block j: rows j k .. j k + k - 1).  X is written, never read.  j ascending, then the columns of Z_j ascending, per entry of X.
__global__ __launch_bounds__(BLK) void cb_combine(const d2_t* __restrict__ Z, long long ldz, int used, const d2_t* __restrict__ Y, d2_t* __restrict__ X,
                                                  long long n, int k) {
  __shared__ d2_t sY[CB_M * CB_KK];
  for (int t = threadIdx.x; t < used * k * k; t += BLK) sY[t] = Y[t];
  __syncthreads();
  const long long total = n * k, stride = (long long)gridDim.x * BLK;
  for (long long idx = (long long)blockIdx.x * BLK + threadIdx.x; idx < total; idx += stride) {
    const long long r = idx / k;
    const int b = (int)(idx - r * k);
    d2_t acc = d2_t{0.0, 0.0};
    for (int j = 0; j < used; ++j) {
      const d2_t* zr = Z + (size_t)j * (size_t)ldz + (size_t)r * k;
      const d2_t* yj = sY + j * k * k;
      for (int a = 0; a < k; ++a) acc += cmul(zr[a], yj[a * k + b]);
    }
    X[idx] = acc;
  }
}

}  // namespace mgcb
