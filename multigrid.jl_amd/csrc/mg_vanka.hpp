// mg_vanka.hpp - kernels of the Vanka cell-block smoother (mg_vanka_*): the device form of the Julia serial path of
// RelaxVankaFacesColor (src/Multigrid/Vanka.jl:383-425; `parallel = false`, l.10 - the red-black C path of Vanka.c never runs).
// Per cell i with unknowns I (2*dim faces [+ its pressure], ascending): r = (b - A y)[I], x[I] += M_i r, where
// M_i = reshape(D[:, i], bs, bs)' is the single-precision w*inv(A[I, I]) promoted to double.
//
// Lane mapping: eight lanes per cell, one lane per ROW of the cell (bs = 4..7 of them busy).  A lane walks its row's
// products in stored order and keeps the sum to itself - no split of a row, so the residual is the serial sum.  The dense
// bs x bs product is taken inside the group of eight: lane t reads M's row t (bs consecutive single-precision values of
// the cell's block, promoted) and fetches r_j from lane j by shuffle, j = 0..bs-1 in order.  One lane per cell would keep
// 4-7 rows of 5-13 entries serial in a lane and make every load of the block strided by bs*bs values; a group of eight
// shares the cell's index arithmetic, reads the block as one contiguous run and keeps 4-7 of 8 lanes busy.
//
// Order independence: a colour's residuals read unknowns that other cells of the SAME colour own (the left-face row of cell
// i1 reaches the right face of cell i1 - 2), so the colour is two launches: vanka_delta reads x only and writes M r into a
// cells x bs buffer; vanka_apply_colour adds a colour's deltas into x (cells of a colour own disjoint unknowns: disjoint
// writes).  The launch boundary is the reference's snapshot y = x.  FULL_VANKA_ADD: y is taken once per call, so the deltas of
// ALL cells are formed once; each iteration is one per-unknown gather (vanka_apply_add) of at most two cells' deltas, the
// lower cell first - the order the reference's linear walk adds them in.  No atomics; identical bits on every run.
//
// Cell and unknown indices are arithmetic on (dim, n, nf): nothing is uploaded but the operator and the blocks.
// T = double, the interleaved complex d2_t or its single twin f2_t (blocks: float or float2, applied conjugated - the stored block
// is the adjoint).  d2_t promotes the block to double; f2_t (a ComplexF32 level: vectors and operator values in float pairs) applies
// it as stored, and every product and sum is single.
//
// From zero (vanka_delta<T, true>): a level entered with x = 0 has r = (b - A 0)[I] = b[I] for the first snapshot, so that pass reads
// b and the block only - no matrix walk.  The general pass on a zero x sums products that are all zeros onto a +0 accumulator, which
// stays +0, and b - (+0) = b bit for bit: both passes write the same deltas.
//
// Blocks of right-hand sides (the _blk kernels at the end; row-major [N][k], 1 <= k <= BLK_KMAX): the group of eight owns one
// (cell, column) pair - group q of a launch serves cell q / k, column q % k - so every rule above holds per column: one lane per
// (row, column) sum, stored order, the dense product j = 0..bs-1 inside the group, delta launch then apply launch, no atomics.  The
// expressions are the ones above, so column c of a block pass has the bits of the one-vector pass on column c.  The k groups of a
// cell are neighbours: the loads of rowptr / col / val and of the dense block hit the same addresses, x[col*k + c] and b[row*k + c]
// are consecutive in c.  delta is [cells][bs][k]; from zero is a property of the whole block.
#pragma once
#include "mg_kernels.hpp"
#include "mg_complex.hpp"

namespace mgk {

struct VankaGeo {
  int dim, ip, bs;          // ip: includePressure
  int n[3];                 // cells per dimension (n[2] = 1 in 2-D)
  int nf[3];                // faces per direction (nf[2] = 0 in 2-D)
  int cells, N;             // prod(n), sum(nf) [+ cells]
};

template <typename T> struct VankaBlk;
template <> struct VankaBlk<double> { typedef float type; };
template <> struct VankaBlk<d2_t> { typedef float2 type; };
template <> struct VankaBlk<f2_t> { typedef float2 type; };

__device__ __forceinline__ double vk_mul(double a, double b) { return a * b; }
__device__ __forceinline__ d2_t vk_mul(d2_t a, d2_t b) { return d2_t{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ f2_t vk_mul(f2_t a, f2_t b) { return f2_t{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
template <typename T> __device__ __forceinline__ T vk_adj(typename VankaBlk<T>::type a);
template <> __device__ __forceinline__ double vk_adj<double>(float a) { return (double)a; }                       // promoted, nothing rounded
template <> __device__ __forceinline__ d2_t vk_adj<d2_t>(float2 a) { return d2_t{(double)a.x, -(double)a.y}; }   // reshape(D)' conjugates
template <> __device__ __forceinline__ f2_t vk_adj<f2_t>(float2 a) { return f2_t{a.x, -a.y}; }                    // as stored: no promotion
__device__ __forceinline__ double vk_shfl8(double a, int j) { return __shfl(a, j, 8); }
__device__ __forceinline__ d2_t vk_shfl8(d2_t a, int j) { return d2_t{__shfl(a.x, j, 8), __shfl(a.y, j, 8)}; }
__device__ __forceinline__ f2_t vk_shfl8(f2_t a, int j) { return f2_t{__shfl(a.x, j, 8), __shfl(a.y, j, 8)}; }

// unknown t of cell (c1, c2, c3), 0-based (getVankaVariablesOfCell, Vanka.jl:45-95)
__device__ __forceinline__ int vanka_unknown(const VankaGeo& G, int c1, int c2, int c3, int t) {
  const int n1 = G.n[0], n2 = G.n[1];
  if (t < 2) return c1 + (n1 + 1) * (c2 + n2 * c3) + t;
  if (t < 4) return G.nf[0] + c1 + n1 * (c2 + (n2 + 1) * c3) + (t == 3 ? n1 : 0);
  const int cell = c1 + n1 * (c2 + n2 * c3);
  if (G.dim == 3 && t < 6) return G.nf[0] + G.nf[1] + cell + (t == 5 ? n1 * n2 : 0);
  return G.nf[0] + G.nf[1] + G.nf[2] + cell;   // the pressure
}

// delta[cell][t] = (M_cell (b - A x)[I])_t for the `count` cells of one colour (parity p[d] in dimension d, m[d] cells
// of that parity per dimension), or for all cells (all != 0: m = n, p ignored).  ZERO: x is known to be zero and is not read
// (r = b[I]); the caller has zero-filled it for the apply pass that follows.
template <typename T, bool ZERO = false>
__global__ __launch_bounds__(BLK) void vanka_delta(VankaGeo G, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                   const T* __restrict__ val, const typename VankaBlk<T>::type* __restrict__ D,
                                                   const T* __restrict__ b, const T* __restrict__ x, T* __restrict__ delta,
                                                   int count, int m1, int m2, int p1, int p2, int p3, int all) {
  const long long gid = (long long)blockIdx.x * BLK + threadIdx.x;
  const int t = (int)(gid & 7);
  const bool live = (gid >> 3) < count;   // (whole groups of eight: the shuffles below run with every lane of a live group)
  int c1 = 0, c2 = 0, c3 = 0;
  if (live) {
    const int g = (int)(gid >> 3);        // < count: 32-bit divisions
    const int k1 = g % m1, q = g / m1, k2 = q % m2, k3 = q / m2;
    c1 = all ? k1 : 2 * k1 + p1;
    c2 = all ? k2 : 2 * k2 + p2;
    c3 = all ? k3 : 2 * k3 + p3;
  }
  const int cell = c1 + G.n[0] * (c2 + G.n[1] * c3);
  T r = T{};
  if (live && t < G.bs) {
    const int row = vanka_unknown(G, c1, c2, c3, t);
    if constexpr (ZERO) {
      r = b[row];
    } else {
      T acc = T{};
      for (int k = rowptr[row], e = rowptr[row + 1]; k < e; ++k) acc += vk_mul(val[k], x[col[k]]);   // stored order, one lane
      r = b[row] - acc;
    }
  }
  T out = T{};
  const typename VankaBlk<T>::type* Mrow = D + (size_t)cell * (size_t)(G.bs * G.bs) + (size_t)(t < G.bs ? t : 0) * (size_t)G.bs;
  for (int j = 0; j < G.bs; ++j) {
    const T rj = vk_shfl8(r, j);
    if (live && t < G.bs) out += vk_mul(vk_adj<T>(Mrow[j]), rj);
  }
  if (live && t < G.bs) delta[(size_t)cell * (size_t)G.bs + (size_t)t] = out;
}

// x[I] += delta[cell] for the cells of one colour
template <typename T>
__global__ __launch_bounds__(BLK) void vanka_apply_colour(VankaGeo G, const T* __restrict__ delta, T* __restrict__ x, int count, int m1,
                                                          int m2, int p1, int p2, int p3) {
  const long long gid = (long long)blockIdx.x * BLK + threadIdx.x;
  const int t = (int)(gid & 7);
  if ((gid >> 3) >= count || t >= G.bs) return;
  const int g = (int)(gid >> 3), q = g / m1;   // < count: 32-bit divisions
  const int c1 = 2 * (g % m1) + p1, c2 = 2 * (q % m2) + p2, c3 = 2 * (q / m2) + p3;
  const int cell = c1 + G.n[0] * (c2 + G.n[1] * c3);
  const int u = vanka_unknown(G, c1, c2, c3, t);
  x[u] = x[u] + delta[(size_t)cell * (size_t)G.bs + (size_t)t];
}

// FULL_VANKA_ADD: x[u] += delta of the lower cell that lists u, then of the upper one (a face has at most two)
template <typename T>
__global__ __launch_bounds__(BLK) void vanka_apply_add(VankaGeo G, const T* __restrict__ delta, T* __restrict__ x) {
  const long long gid = (long long)blockIdx.x * BLK + threadIdx.x;
  if (gid >= G.N) return;   // (compared before narrowing: N may be within BLK of 2^31)
  const int u = (int)gid;
  const int n1 = G.n[0], n2 = G.n[1], n3 = G.n[2];
  int lo = -1, hi = -1, tlo = 0, thi = 0;   // cells and the unknown's slot in each
  if (u < G.nf[0]) {
    const int f = u % (n1 + 1), rest = u / (n1 + 1);   // rest = c2 + n2 * c3
    if (f >= 1) { lo = (f - 1) + n1 * rest; tlo = 1; }
    if (f < n1) { hi = f + n1 * rest; thi = 0; }
  } else if (u < G.nf[0] + G.nf[1]) {
    const int v = u - G.nf[0];
    const int c1 = v % n1, f = (v / n1) % (n2 + 1), c3 = v / (n1 * (n2 + 1));
    if (f >= 1) { lo = c1 + n1 * ((f - 1) + n2 * c3); tlo = 3; }
    if (f < n2) { hi = c1 + n1 * (f + n2 * c3); thi = 2; }
  } else if (u < G.nf[0] + G.nf[1] + G.nf[2]) {
    const int v = u - G.nf[0] - G.nf[1];
    const int inplane = v % (n1 * n2), f = v / (n1 * n2);
    if (f >= 1) { lo = inplane + n1 * n2 * (f - 1); tlo = 5; }
    if (f < n3) { hi = inplane + n1 * n2 * f; thi = 4; }
  } else {
    lo = u - G.nf[0] - G.nf[1] - G.nf[2];
    tlo = G.bs - 1;
  }
  T v = x[u];
  if (lo >= 0) v = v + delta[(size_t)lo * (size_t)G.bs + (size_t)tlo];
  if (hi >= 0) v = v + delta[(size_t)hi * (size_t)G.bs + (size_t)thi];
  x[u] = v;
}

// ---- blocks of right-hand sides: row-major [N][k], 1 <= k <= BLK_KMAX ------------------------------------------------------------
// The eight-lane group stays and owns one (cell, column) pair: group q serves the cell q / k of the launch and the column q % k, so a
// lane still owns one (row, column) sum, walks the row's products in stored order and takes the dense product j = 0..bs-1 inside its
// group.  Neighbouring groups (the k columns of a cell) read the same rowptr / col / val / block addresses - one fetch serves them -
// and x[col*k + c], b[row*k + c] are consecutive in c.  The expressions are those of the one-vector kernels, so column c of a block
// pass holds the bits the one-vector kernels give on column c alone; k = 1 is the one-vector pass.  delta is [cells][bs][k].
// cells * 8 * k and N * k are formed in 64 bits and compared before anything is narrowed.
template <typename T, bool ZERO = false>
__global__ __launch_bounds__(BLK) void vanka_delta_blk(VankaGeo G, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                       const T* __restrict__ val, const typename VankaBlk<T>::type* __restrict__ D,
                                                       const T* __restrict__ b, const T* __restrict__ x, T* __restrict__ delta, int k,
                                                       int count, int m1, int m2, int p1, int p2, int p3, int all) {
  const long long gid = (long long)blockIdx.x * BLK + threadIdx.x;
  const int t = (int)(gid & 7);
  const long long grp = gid >> 3;
  const bool live = grp < (long long)count * k;   // (whole groups of eight: the shuffles below run with every lane of a live group)
  int c1 = 0, c2 = 0, c3 = 0, c = 0;
  if (live) {
    const int g = (int)(grp / k);         // < count
    c = (int)(grp % k);
    const int k1 = g % m1, q = g / m1, k2 = q % m2, k3 = q / m2;
    c1 = all ? k1 : 2 * k1 + p1;
    c2 = all ? k2 : 2 * k2 + p2;
    c3 = all ? k3 : 2 * k3 + p3;
  }
  const int cell = c1 + G.n[0] * (c2 + G.n[1] * c3);
  T r = T{};
  if (live && t < G.bs) {
    const int row = vanka_unknown(G, c1, c2, c3, t);
    if constexpr (ZERO) {
      r = b[(size_t)row * (size_t)k + (size_t)c];
    } else {
      T acc = T{};
      for (int e = rowptr[row], end = rowptr[row + 1]; e < end; ++e)
        acc += vk_mul(val[e], x[(size_t)col[e] * (size_t)k + (size_t)c]);   // stored order, one lane
      r = b[(size_t)row * (size_t)k + (size_t)c] - acc;
    }
  }
  T out = T{};
  const typename VankaBlk<T>::type* Mrow = D + (size_t)cell * (size_t)(G.bs * G.bs) + (size_t)(t < G.bs ? t : 0) * (size_t)G.bs;
  for (int j = 0; j < G.bs; ++j) {
    const T rj = vk_shfl8(r, j);
    if (live && t < G.bs) out += vk_mul(vk_adj<T>(Mrow[j]), rj);
  }
  if (live && t < G.bs) delta[((size_t)cell * (size_t)G.bs + (size_t)t) * (size_t)k + (size_t)c] = out;
}

// x[I][c] += delta[cell][.][c] for the cells of one colour
template <typename T>
__global__ __launch_bounds__(BLK) void vanka_apply_colour_blk(VankaGeo G, const T* __restrict__ delta, T* __restrict__ x, int k, int count,
                                                              int m1, int m2, int p1, int p2, int p3) {
  const long long gid = (long long)blockIdx.x * BLK + threadIdx.x;
  const int t = (int)(gid & 7);
  const long long grp = gid >> 3;
  if (grp >= (long long)count * k || t >= G.bs) return;
  const int g = (int)(grp / k), c = (int)(grp % k), q = g / m1;
  const int c1 = 2 * (g % m1) + p1, c2 = 2 * (q % m2) + p2, c3 = 2 * (q / m2) + p3;
  const int cell = c1 + G.n[0] * (c2 + G.n[1] * c3);
  const size_t u = (size_t)vanka_unknown(G, c1, c2, c3, t) * (size_t)k + (size_t)c;
  x[u] = x[u] + delta[((size_t)cell * (size_t)G.bs + (size_t)t) * (size_t)k + (size_t)c];
}

// FULL_VANKA_ADD on a block: one lane per (unknown, column), the lower cell's delta first
template <typename T>
__global__ __launch_bounds__(BLK) void vanka_apply_add_blk(VankaGeo G, const T* __restrict__ delta, T* __restrict__ x, int k) {
  const long long gid = (long long)blockIdx.x * BLK + threadIdx.x;
  if (gid >= (long long)G.N * k) return;   // (compared before narrowing)
  const int u = (int)(gid / k), c = (int)(gid % k);
  const int n1 = G.n[0], n2 = G.n[1], n3 = G.n[2];
  int lo = -1, hi = -1, tlo = 0, thi = 0;   // cells and the unknown's slot in each
  if (u < G.nf[0]) {
    const int f = u % (n1 + 1), rest = u / (n1 + 1);   // rest = c2 + n2 * c3
    if (f >= 1) { lo = (f - 1) + n1 * rest; tlo = 1; }
    if (f < n1) { hi = f + n1 * rest; thi = 0; }
  } else if (u < G.nf[0] + G.nf[1]) {
    const int v = u - G.nf[0];
    const int c1 = v % n1, f = (v / n1) % (n2 + 1), c3 = v / (n1 * (n2 + 1));
    if (f >= 1) { lo = c1 + n1 * ((f - 1) + n2 * c3); tlo = 3; }
    if (f < n2) { hi = c1 + n1 * (f + n2 * c3); thi = 2; }
  } else if (u < G.nf[0] + G.nf[1] + G.nf[2]) {
    const int v = u - G.nf[0] - G.nf[1];
    const int inplane = v % (n1 * n2), f = v / (n1 * n2);
    if (f >= 1) { lo = inplane + n1 * n2 * (f - 1); tlo = 5; }
    if (f < n3) { hi = inplane + n1 * n2 * f; thi = 4; }
  } else {
    lo = u - G.nf[0] - G.nf[1] - G.nf[2];
    tlo = G.bs - 1;
  }
  T v = x[(size_t)gid];
  if (lo >= 0) v = v + delta[((size_t)lo * (size_t)G.bs + (size_t)tlo) * (size_t)k + (size_t)c];
  if (hi >= 0) v = v + delta[((size_t)hi * (size_t)G.bs + (size_t)thi) * (size_t)k + (size_t)c];
  x[(size_t)gid] = v;
}

// ---- the cells' blocks built on the device: setupVankaFacesPreconditioner (Vanka.jl:294-370) from the resident operator -------------
// vanka_build_blocks<T>: one launch per level, the eight-lane group of the apply kernels per cell.  Lane t owns row t of [Acc | I]:
// it gathers Acc[t, :] = A[I_t, I] from its own CSR row (one compare of every stored column with the cell's bs unknowns; an absent
// entry stays zero, of a repeated one the first counts), applies the variant's edit, and the group inverts by Gauss-Jordan with
// partial pivoting: per column the largest squared modulus among the rows not yet used (three exchange steps inside the group, the
// lowest row on ties), the rows exchanged, the pivot row scaled by the pivot's reciprocal and taken out of every other row.  Rows
// travel between lanes by shuffles of registers that every loop below indexes with compile-time constants (the loops are unrolled to
// VK_MAXBS and cut by the group-uniform bs): nothing is indexed dynamically, nothing goes to scratch or LDS.  All arithmetic is in
// double (a float-pair operator is widened on load); the resident values are A's own (conjugated once at upload), i.e. what the host
// function reads.  Lane t then scales its row of the inverse (scale_t below) and writes conj(Minv[t, j]) in single precision to entry
// j + t*bs of the cell's column - the LocalBlocks layout, the cell's bs*bs values one contiguous run of the group's stores.
// A pivot whose squared modulus is zero or not finite marks the cell: flag[0] counts such cells, flag[1] keeps INT_MAX - the lowest one (integer
// atomics on a zero-filled pair), and the cell's block is not written.  No floating-point atomics: the same bits on every run.
constexpr int VK_MAXBS = 7;

struct VankaBuild {
  int type;          // 1 FULL_VANKA_RB, 3 ECON_VANKA_RB, 5 FULL_VANKA_ADD
  int scalar;        // w is one number (nw = 1): types 1 and 3 replace the leading (bs-1)x(bs-1) part of Acc by its diagonal
  double w0, w1;     // W = w0 everywhere, w1 on the pressure row of a pair (scalar: w1 = w0)
};

template <typename T> struct VankaWide;   // the type the elimination runs in
template <> struct VankaWide<double> { typedef double type; };
template <> struct VankaWide<d2_t> { typedef d2_t type; };
template <> struct VankaWide<f2_t> { typedef d2_t type; };
__device__ __forceinline__ double vb_widen(double a) { return a; }
__device__ __forceinline__ d2_t vb_widen(d2_t a) { return a; }
__device__ __forceinline__ d2_t vb_widen(f2_t a) { return d2_t{(double)a.x, (double)a.y}; }
__device__ __forceinline__ double vb_abs2(double a) { return a * a; }
__device__ __forceinline__ double vb_abs2(d2_t a) { return a.x * a.x + a.y * a.y; }
__device__ __forceinline__ double vb_recip(double p, double) { return 1.0 / p; }
__device__ __forceinline__ d2_t vb_recip(d2_t p, double m2) { return d2_t{p.x / m2, -p.y / m2}; }
__device__ __forceinline__ double vb_scale(double s, double a) { return s * a; }
__device__ __forceinline__ d2_t vb_scale(double s, d2_t a) { return d2_t{s * a.x, s * a.y}; }
__device__ __forceinline__ double vb_one(double) { return 1.0; }
__device__ __forceinline__ d2_t vb_one(d2_t) { return d2_t{1.0, 0.0}; }
__device__ __forceinline__ float vb_store(double a) { return (float)a; }
__device__ __forceinline__ float2 vb_store(d2_t a) { return make_float2((float)a.x, -(float)a.y); }   // the stored block is the adjoint

template <typename T>
__global__ __launch_bounds__(BLK) void vanka_build_blocks(VankaGeo G, VankaBuild P, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                          const T* __restrict__ val, typename VankaBlk<T>::type* __restrict__ D,
                                                          int* __restrict__ flag) {
  typedef typename VankaWide<T>::type W;
  const long long gid = (long long)blockIdx.x * BLK + threadIdx.x;
  const int t = (int)(gid & 7);
  const bool live = (gid >> 3) < G.cells;   // (whole groups of eight: every lane of a live group runs the shuffles below)
  const int bs = G.bs;
  const int cell = live ? (int)(gid >> 3) : 0;
  const int c1 = cell % G.n[0], q = cell / G.n[0], c2 = q % G.n[1], c3 = q / G.n[1];
  const bool mine = live && t < bs;
  // row t of [Acc | I]; the lanes past bs hold rows of the identity, which no pivot search considers
  W a[VK_MAXBS], v[VK_MAXBS];
#pragma unroll
  for (int j = 0; j < VK_MAXBS; ++j) {
    a[j] = W{};
    v[j] = j == t ? vb_one(W{}) : W{};
  }
  if (mine) {
    int I[VK_MAXBS];
#pragma unroll
    for (int j = 0; j < VK_MAXBS; ++j) I[j] = j < bs ? vanka_unknown(G, c1, c2, c3, j) : -1;
    const int row = vanka_unknown(G, c1, c2, c3, t);
    for (int e = rowptr[row + 1] - 1, e0 = rowptr[row]; e >= e0; --e) {   // backwards: of a repeated column the first entry stays
      const int c = col[e];
      const W x = vb_widen(val[e]);
#pragma unroll
      for (int j = 0; j < VK_MAXBS; ++j)
        if (c == I[j]) a[j] = x;
    }
    // the variant's edit of Acc (Vanka.jl:327-362)
    if (P.scalar && (P.type == 1 || P.type == 3) && t < bs - 1) {
#pragma unroll
      for (int j = 0; j < VK_MAXBS; ++j) {
        if (j < bs - 1 && j != t) a[j] = W{};
        if (j == t && P.type == 3) a[j] = a[j] / P.w0;
      }
    }
  }
  bool bad = false;
#pragma unroll
  for (int k = 0; k < VK_MAXBS; ++k) {
    if (k >= bs) break;   // (uniform)
    // the pivot: largest squared modulus of column k among rows k .. bs-1, the lowest row on ties
    double best = (t >= k && t < bs) ? vb_abs2(a[k]) : -1.0;
    if (best != best) best = __builtin_inf();   // (a NaN entry is chosen and then refused below)
    int at = t;
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
      const double ob = __shfl_xor(best, o, 8);
      const int oa = __shfl_xor(at, o, 8);
      if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
    }
    if (!(best > 0.0) || best == __builtin_inf()) bad = true;
    // rows k and `at` change places; the pivot row is scaled and taken out of the others
    W pa[VK_MAXBS], pv[VK_MAXBS];
#pragma unroll
    for (int j = 0; j < VK_MAXBS; ++j) {
      const W ka = vk_shfl8(a[j], k), kv = vk_shfl8(v[j], k);
      pa[j] = vk_shfl8(a[j], at);
      pv[j] = vk_shfl8(v[j], at);
      if (t == at) { a[j] = ka; v[j] = kv; }
    }
    const W rp = vb_recip(pa[k], best);
#pragma unroll
    for (int j = 0; j < VK_MAXBS; ++j) {
      pa[j] = vk_mul(rp, pa[j]);
      pv[j] = vk_mul(rp, pv[j]);
    }
    if (t == k) {
#pragma unroll
      for (int j = 0; j < VK_MAXBS; ++j) { a[j] = pa[j]; v[j] = pv[j]; }
    } else {
      const W f = a[k];
#pragma unroll
      for (int j = 0; j < VK_MAXBS; ++j) {
        a[j] = a[j] - vk_mul(f, pa[j]);
        v[j] = v[j] - vk_mul(f, pv[j]);
      }
    }
  }
  if (!live) return;
  if (bad) {
    if (t == 0) {
      atomicAdd(&flag[0], 1);
      atomicMax(&flag[1], INT_MAX - cell);
    }
    return;
  }
  if (t >= bs) return;
  // the damping of row t: W_t (type 1), nothing (type 3), t_t * W_t with t_t = 1/2 on a face shared with a neighbour (type 5)
  double s = 1.0;
  if (P.type != 3) {
    const bool pressure = G.ip && t == bs - 1;
    s = pressure ? P.w1 : P.w0;
    if (P.type == 5 && !pressure) {
      const int d = t >> 1, c = d == 0 ? c1 : d == 1 ? c2 : c3, nd = d == 0 ? G.n[0] : d == 1 ? G.n[1] : G.n[2];
      const bool boundary = (t & 1) ? c == nd - 1 : c == 0;
      s = (boundary ? 1.0 : 0.5) * s;
    }
  }
  typename VankaBlk<T>::type* out = D + (size_t)cell * (size_t)(bs * bs) + (size_t)t * (size_t)bs;
#pragma unroll
  for (int j = 0; j < VK_MAXBS; ++j)
    if (j < bs) out[j] = vb_store(vb_scale(s, v[j]));   // (s = 1 is exact)
}

}  // namespace mgk
