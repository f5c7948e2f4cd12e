// mg_complex.hpp - gfx950 kernels of the ComplexF64 (CF64) cycle and of its single-precision form (CF32: the same kernels on
// float pairs, see f2_t below): generic CSR only; the conjugate transpose of an operator in HBM (cx_adj_*: adjointHierarchy); complex
// hybrid Kaczmarz and the Float32 / ComplexF32 one (hybrid_kaczmarz_s); the chip-wide complex triangular solve of the factor applier (cx_sptrsv_*, cx_tri_*, at the end).
//
// Complex values are interleaved (re, im) doubles - Julia ComplexF64, numpy complex128, hipDoubleComplex - and are
// loaded as one 16-byte d2_t.  The operator A of a CF64 handle is stored conjugated at upload (nzval of the
// reference's AT, conj'd once), so every kernel here computes a plain sum of products: y_i = sum_k val_k * x[col_k]
// is the reference's mul!(y, adjoint(AT), x) (SpMatMul.jl:9).  P and R stay real (MGsetup.jl:80-81) and are applied
// to complex vectors by the same kernel with a real value stream.
//
// Streaming layout (the complex form of csr_stream_spmv, mg_kernels.hpp): the host cuts the rows into row blocks
// whose non-zeros fit one LDS chunk of CX_CHUNK products; a workgroup issues every load of its block up front (16 B
// per lane per complex value, coalesced), stages the products in LDS, and ONE lane per row sums its row's products
// in stored order, then applies the fused epilogue.  Workgroups are banded per XCD (xcd_band).  A row longer than a
// chunk has a block of its own and the whole workgroup strides over it.
// Epilogues: AXPBY, RESID (optionally also z1 = d.*r), SMOOTH, and GRAM - one step of the FGMRES relaxation (Jac-GMRES smoothing,
// K-cycle; ComplexF64, and ComplexF32 where the handle's option single_kcycle is set): w = A z_j stored as column j of AZ, the next direction d.*w, and the per-row-block partial sums of
// column j of H = (AZ)'(AZ) and of xi[j] = dot(w, r0), see CxVecArgsT.  cx_csr_stream_spmm has the same mode for a block of right-hand
// sides taken as ONE long vector (the handle's option kcycle_blocks): one H, one xi for the whole block.
// CGDOT - one Arnoldi step of the GMRES coarsest solve (coarseSolveType "GMRES"; ComplexF64 only): w = A z_i stored as the next
// basis vector, and the per-row-block partial sums of dot(v_0, w), the first coefficient of the Gram-Schmidt chain that follows
// (mg_cxvec.hpp).
// Blocks of right-hand sides (row-major [n][nrhs]) run on the same row blocks: cx_csr_stream_spmm stages the matrix stream itself in
// LDS and lets pow2 >= nrhs lanes per row walk it (below, behind the vector kernel).
#pragma once
#include "mg_kernels.hpp"

namespace mgk {

constexpr int CX_ITEMS = 4;                 // complex products per thread per chunk
constexpr int CX_CHUNK = BLK * CX_ITEMS;    // 1024 products: 16 KiB of LDS per workgroup in double, 8 KiB in single (one row-block
                                            // scheme for both precisions: the widened copy of a single operator keeps its blocks)

// A ComplexF32 (CF32) hierarchy runs the same kernels on (re, im) float pairs: every kernel of the cycle below is written once
// over the pair type C (d2_t or f2_t) with its scalar cx_scalar<C>.  Products and row sums are formed in C's precision, in stored
// order (the reference's arithmetic for VAL = ComplexF32); the partials of ||r||^2 are double for both.
// (f2_t: mg_kernels.hpp, beside d2_t)
template <typename C> struct cx_scalar;
template <> struct cx_scalar<d2_t> { typedef double type; };
template <> struct cx_scalar<f2_t> { typedef float type; };

__device__ __forceinline__ d2_t cmul(d2_t a, d2_t b) { return d2_t{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ d2_t cmul(double a, d2_t b) { return d2_t{a * b.x, a * b.y}; }
__device__ __forceinline__ f2_t cmul(f2_t a, f2_t b) { return f2_t{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ f2_t cmul(float a, f2_t b) { return f2_t{a * b.x, a * b.y}; }
__device__ __forceinline__ d2_t cdiv(d2_t a, d2_t b) {
  const double s = b.x * b.x + b.y * b.y;
  return d2_t{(a.x * b.x + a.y * b.y) / s, (a.y * b.x - a.x * b.y) / s};
}
__device__ __forceinline__ double cabs2(d2_t a) { return a.x * a.x + a.y * a.y; }
__device__ __forceinline__ double cabs2(f2_t a) { return (double)a.x * (double)a.x + (double)a.y * (double)a.y; }   // exact products
// a value widened to double: every product of two widened singles is exact
__device__ __forceinline__ d2_t cwide(d2_t a) { return a; }
__device__ __forceinline__ d2_t cwide(f2_t a) { return d2_t{(double)a.x, (double)a.y}; }
__device__ __forceinline__ d2_t shfl_xor_v(d2_t a, int o) { return d2_t{__shfl_xor(a.x, o), __shfl_xor(a.y, o)}; }
__device__ __forceinline__ f2_t shfl_xor_v(f2_t a, int o) { return f2_t{__shfl_xor(a.x, o), __shfl_xor(a.y, o)}; }

// the value stream of an operator: complex (A, conj'd at upload) or real (P, R)
template <typename PTR, typename VT>
struct CxCsrDev {
  const PTR* rowptr;   // n_rows+1, 0-based
  const int* colidx;   // nnz
  const VT* val;       // nnz
  const int* blk_row;  // nblocks+1
  int nblocks;
  int n_rows;
};

// GRAM (both pair types; cx_csr_stream_spmm: the same step on a block taken as one long vector, option kcycle_blocks): step j of FGMRES_relaxation (FGMRES.jl:82-104) in the walk that computes w = A z_j.
// The mode follows mgk::Mode (AXPBY, RESID, SMOOTH) and is served by no other kernel.
constexpr int GRAM = 3;
constexpr int GRAM_MAXV = 8;                       // directions of one relaxation at most (mgcv::MAXV, the width of the combination pass)
constexpr int GRAM_NS = 2 * GRAM_MAXV + 1;         // real scalars of a step at most: 2 j + 3 for j <= 7
// CGDOT (cx_csr_stream_spmv only, ComplexF64): w = A z stored (y) with the partials of dot(v_0, w) = sum conj(v_0[row]) w[row]
// (v_0 in r0) at gpart[bid] (re) and gpart[nblocks + bid] (im) - GRAM's reduction on two scalars: lane registers, wavefront
// shuffles, the workgroup's LDS, one partial per row block, no atomics, the same bits on every run.
constexpr int CGDOT = 4;

template <typename C>
struct CxVecArgsT {
  const C* x;      // gathered vector  [n_cols]
  C* y;            // output           [n_rows]   (GRAM: w, column j of AZ)
  const C* b;      // RESID / SMOOTH   [n_rows]
  const C* d;      // SMOOTH: relaxPrec [n_rows]  (RESID with z1, GRAM with znext: the Jacobi preconditioner MM, MGcycle.jl:36-38)
  double* sumsq;   // optional: per-row-block sum of |out|^2 (summed by sum_final)
  C alpha;         // AXPBY
  C beta;          // AXPBY (beta == 0: y is not read)
  int beta_zero;
  C* z1;           // RESID, optional: also d.*r, the first direction of the relaxation that follows
  // GRAM: w = A z_j is stored (y), the next direction d.*w is stored (znext, optional), and every row block leaves the partial sums of
  //   |w[row]|^2                      (H[j][j], real:    scalar 0)
  //   conj(w[row]) r0[row]            (xi[j], complex:   scalars 1, 2)
  //   conj(AZ_i[row]) w[row], i < j   (H[i][j], complex: scalars 3 + 2 i, 4 + 2 i)
  // at gpart[c * nblocks + bid], c < 2 j + 3
  const C* az;     // AZ, column-major: column i at az + i * ldz
  const C* r0;
  C* znext;
  double* gpart;
  long long ldz;
  int gj;
};
typedef CxVecArgsT<d2_t> CxVecArgs;

// pb: beta*y (AXPBY) or b (RESID, SMOOTH); px, pd: the row's x and d (SMOOTH; x is the gathered vector itself)
template <int MODE, typename C>
__device__ __forceinline__ C cx_epilogue(const CxVecArgsT<C>& v, C acc, C pb, C pd, C px) {
  if (MODE == AXPBY) return cmul(v.alpha, acc) + pb;
  if (MODE == RESID) return pb - acc;
  if (MODE == GRAM || MODE == CGDOT) return acc;
  return px + cmul(pd, pb - acc);   // SMOOTH: x + d.*(b - A x)   (MGcycle.jl:129-131)
}

template <int MODE, typename C>
__device__ __forceinline__ void cx_operands(const CxVecArgsT<C>& v, int row, C& pb, C& pd, C& px) {
  if (MODE == AXPBY) {
    if (!v.beta_zero) pb = cmul(v.beta, v.y[row]);
  } else if (MODE == GRAM) {
    pb = v.r0[row];
    if (v.znext) pd = v.d[row];
  } else if (MODE == CGDOT) {
    pb = v.r0[row];
  } else {
    pb = v.b[row];
  }
  if (MODE == SMOOTH) {
    pd = v.d[row];
    px = v.x[row];
  }
  if (MODE == RESID && v.z1) pd = v.d[row];
}

// the Gram scalars of one row: s[0 .. 2 j + 3) for w = (A z_j)[row], azv[i] = AZ_i[row], r0v = r0[row].
// The operands are widened to double BEFORE they are multiplied (cwide), so on a ComplexF32 hierarchy every product is exact and only
// the sums round - in double.  (The reference forms H in ComplexF32, where the estimate rn = sqrt|t'Ht - 2t'xi + ||r0||^2| cancels
// down to about sqrt(2^-24) ||r0|| and the break at rn < 1e-5 is noise; see the README.)
template <typename C>
__device__ __forceinline__ void cx_gram_row(double* s, int j, const C* azv, C wv, C r0v) {
  const d2_t w = cwide(wv), r = cwide(r0v);
  s[0] = cabs2(wv);
  s[1] = w.x * r.x + w.y * r.y;
  s[2] = w.x * r.y - w.y * r.x;
#pragma unroll
  for (int i = 0; i < GRAM_MAXV - 1; ++i)
    if (i < j) {
      const d2_t a = cwide(azv[i]);
      s[3 + 2 * i] = a.x * w.x + a.y * w.y;
      s[4 + 2 * i] = a.x * w.y - a.y * w.x;
    }
}

template <int MODE, typename PTR, typename VT, typename C>
__global__ __launch_bounds__(BLK) void cx_csr_stream_spmv(CxCsrDev<PTR, VT> A, CxVecArgsT<C> v) {
  typedef typename cx_scalar<C>::type T;
  __shared__ C prod[CX_CHUNK];
  __shared__ int srow[MAXROWS + 1];
  __shared__ double red[(MODE == GRAM ? GRAM_NS : 2) * (BLK / 64)];

  const int tid = threadIdx.x;
  const int bid = xcd_band(blockIdx.x, A.nblocks);
  const int r0 = A.blk_row[bid];
  const int r1 = A.blk_row[bid + 1];
  const int nrows = r1 - r0;
  const PTR k0 = A.rowptr[r0];
  const PTR k1 = A.rowptr[r1];

  if (nrows == 1 && (k1 - k0) > CX_CHUNK) {
    // one row longer than a chunk: the whole workgroup strides over it
    C acc = C{};
    for (PTR k = k0 + tid; k < k1; k += BLK) acc += cmul(A.val[k], v.x[A.colidx[k]]);
    for (int o = 32; o > 0; o >>= 1) acc += shfl_xor_v(acc, o);
    if ((tid & 63) == 0) {   // (a float travels through a double slot unchanged)
      red[2 * (tid >> 6)] = acc.x;
      red[2 * (tid >> 6) + 1] = acc.y;
    }
    __syncthreads();
    if (tid == 0) {
      C s = C{};
      for (int w = 0; w < BLK / 64; ++w) s += C{(T)red[2 * w], (T)red[2 * w + 1]};
      C pb = C{}, pd = pb, px = pb;
      cx_operands<MODE>(v, r0, pb, pd, px);
      const C o = cx_epilogue<MODE>(v, s, pb, pd, px);
      v.y[r0] = o;
      if (v.sumsq) v.sumsq[bid] = cabs2(o);
      if (MODE == RESID && v.z1) v.z1[r0] = cmul(pd, o);
      if constexpr (MODE == GRAM) {   // the block's only row: its scalars are the block's partials
        if (v.znext) v.znext[r0] = cmul(pd, o);
        const int j = v.gj;
        C azv[GRAM_MAXV - 1];
#pragma unroll
        for (int i = 0; i < GRAM_MAXV - 1; ++i) azv[i] = i < j ? v.az[(size_t)i * v.ldz + r0] : C{};
        double gs[GRAM_NS];
#pragma unroll
        for (int c = 0; c < GRAM_NS; ++c) gs[c] = 0.0;
        cx_gram_row(gs, j, azv, o, pb);
#pragma unroll
        for (int c = 0; c < GRAM_NS; ++c)
          if (c < 2 * j + 3) v.gpart[(size_t)c * A.nblocks + bid] = gs[c];
      }
      if constexpr (MODE == CGDOT) {
        v.gpart[bid] = pb.x * o.x + pb.y * o.y;
        v.gpart[(size_t)A.nblocks + bid] = pb.x * o.y - pb.y * o.x;
      }
    }
    return;
  }

  // ---- every global load up front: matrix stream, row pointers, epilogue operands ----------------
  VT va[CX_ITEMS];
  int ca[CX_ITEMS];
#pragma unroll
  for (int it = 0; it < CX_ITEMS; ++it) {
    const PTR idx = k0 + it * BLK + tid;
    if (idx < k1) {
      va[it] = A.val[idx];
      ca[it] = A.colidx[idx];
    } else {
      va[it] = VT{};
      ca[it] = 0;
    }
  }
  if (tid <= nrows) srow[tid] = (int)(A.rowptr[r0 + tid] - k0);
  if (tid == 0 && nrows == MAXROWS) srow[MAXROWS] = (int)(k1 - k0);
  const bool owner = tid < nrows;
  C pb = C{}, pd = pb, px = pb;
  if (owner) cx_operands<MODE>(v, r0 + tid, pb, pd, px);
  C azv[MODE == GRAM ? GRAM_MAXV - 1 : 1];
  if constexpr (MODE == GRAM) {   // the row's entries of the columns of AZ before j
#pragma unroll
    for (int i = 0; i < GRAM_MAXV - 1; ++i) azv[i] = (owner && i < v.gj) ? v.az[(size_t)i * v.ldz + r0 + tid] : C{};
  }
  // ---- gather x and stage the products -----------------------------------------------------------
#pragma unroll
  for (int it = 0; it < CX_ITEMS; ++it) {
    const PTR idx = k0 + it * BLK + tid;
    if (idx < k1) prod[it * BLK + tid] = cmul(va[it], v.x[ca[it]]);
  }
  __syncthreads();
  // ---- one lane per row: the row's products in stored order, fused epilogue ------------------------
  C outv = C{};
  if (owner) {
    C acc = C{};
    const int s = srow[tid], e = srow[tid + 1];
    for (int k = s; k < e; ++k) acc += prod[k];
    outv = cx_epilogue<MODE>(v, acc, pb, pd, px);
    v.y[r0 + tid] = outv;
    if (MODE == RESID && v.z1) v.z1[r0 + tid] = cmul(pd, outv);
    if (MODE == GRAM && v.znext) v.znext[r0 + tid] = cmul(pd, outv);
  }
  if constexpr (MODE == GRAM) {
    // 2 j + 3 scalars: lane registers (a lane owns one row; the others add zeros), wavefront shuffles, the workgroup's LDS, one
    // partial per scalar and row block - no atomics, the same bits on every run
    const int j = v.gj, ns = 2 * j + 3;
    double gs[GRAM_NS];
#pragma unroll
    for (int c = 0; c < GRAM_NS; ++c) gs[c] = 0.0;
    cx_gram_row(gs, j, azv, outv, pb);   // (outv, pb and azv are zero in a lane without a row)
#pragma unroll
    for (int c = 0; c < GRAM_NS; ++c)
      if (c < ns) {   // (uniform)
        double t = gs[c];
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
        if ((tid & 63) == 0) red[c * (BLK / 64) + (tid >> 6)] = t;
      }
    __syncthreads();
    if (tid < ns) {
      double t = 0.0;
      for (int w = 0; w < BLK / 64; ++w) t += red[tid * (BLK / 64) + w];
      v.gpart[(size_t)tid * A.nblocks + bid] = t;
    }
    return;
  }
  if constexpr (MODE == CGDOT) {   // (outv and pb are zero in a lane without a row)
    double t0 = pb.x * outv.x + pb.y * outv.y, t1 = pb.x * outv.y - pb.y * outv.x;
    for (int o = 32; o > 0; o >>= 1) {
      t0 += __shfl_xor(t0, o);
      t1 += __shfl_xor(t1, o);
    }
    if ((tid & 63) == 0) {
      red[tid >> 6] = t0;
      red[(BLK / 64) + (tid >> 6)] = t1;
    }
    __syncthreads();
    if (tid < 2) {
      double t = 0.0;
      for (int w = 0; w < BLK / 64; ++w) t += red[tid * (BLK / 64) + w];
      v.gpart[(size_t)tid * A.nblocks + bid] = t;
    }
    return;
  }
  if (v.sumsq) {   // ||r||^2 = sum |r_i|^2 (SolveFuncs.jl:30): a deterministic per-block partial, summed by sum_final
    double sq = cabs2(outv);
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
    if ((tid & 63) == 0) red[tid >> 6] = sq;
    __syncthreads();
    if (tid == 0) {
      double t = 0.0;
      for (int w = 0; w < BLK / 64; ++w) t += red[w];
      v.sumsq[bid] = t;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Blocks of right-hand sides: Y = epilogue(A * X) for row-major blocks [n][nrhs] (1 <= nrhs <= BLK_KMAX), on the SAME row blocks
// as cx_csr_stream_spmv.  The matrix stream - values AND column indices - is staged in LDS once per workgroup (coalesced loads,
// all issued up front: 16 + 4 KiB for complex A, 8 + 4 KiB for real P / R, half the value bytes in single) and is then walked
// by nrhs columns, so the operator is read from HBM once per block instead of once per column.
// Lane mapping: work item t = row * G + column, G = pow2 >= nrhs; a workgroup takes its items BLK at a time, so G consecutive
// lanes own one row (lanes with column >= nrhs idle) and consecutive lane groups own consecutive rows.  Every lane walks its
// row from LDS in STORED order and sums in its own register: each (row, column) is one lane's sum in a fixed order - the same
// bits on every run, whatever the other columns hold.  The LDS reads of one row's entry are the same address in its G lanes
// (a broadcast); the 64 / G rows of a wavefront read addresses one row length apart.  For rows of equal odd length (7- and
// 27-point operators: 7 or 27 slots of 16 B for ds_read_b128, banks (a/4) mod 64; 7 or 27 dwords for the indices, mod 32) the
// rows of a lane group fall on distinct banks; rows of even length cost up to gcd(length, 16)-way conflicts, as they do for
// the one-lane-per-row sum of the vector kernel.  The gather of X for one entry is one contiguous 16 * nrhs-byte segment
// across the G lanes (8 * nrhs in single).  d[row] of SMOOTH is shared by the columns.  sumsq: the per-row-block partial of
// sum |out|^2 over ALL columns (solveMG's Frobenius norm).  A row longer than a chunk: BLK / G lane groups stride over it,
// and the per-column partial sums are added in lane-group order by one lane per column.
// RESID optionally stores z1 = d[row] * r as well (the first direction of the FGMRES relaxation that follows).  GRAM: step j of that
// relaxation on the block as ONE long vector of length n * nrhs (FGMRES.jl:51-53): W = A Z_j is stored (y: block j of AZ, blocks
// ldz = n * nrhs apart), znext = d[row] * W optionally, and every row block leaves the 2 j + 3 partial sums of CxVecArgsT over all its
// rows and columns in the vector form's slots.
// ------------------------------------------------------------------------------------------------
template <int MODE, typename C>
__device__ __forceinline__ void cx_operands_blk(const CxVecArgsT<C>& v, int row, size_t e, C& pb, C& pd, C& px) {
  if (MODE == AXPBY) {
    if (!v.beta_zero) pb = cmul(v.beta, v.y[e]);
  } else {
    pb = MODE == GRAM ? v.r0[e] : v.b[e];
  }
  if (MODE == SMOOTH) {
    pd = v.d[row];
    px = v.x[e];
  }
  if ((MODE == RESID && v.z1) || (MODE == GRAM && v.znext)) pd = v.d[row];   // (shared by the columns, as SMOOTH shares it)
}

// the Gram scalars of one (row, column) of a block added to the lane's own sums gs[0 .. 2 j + 3): w = W[row][c], the entries of the
// earlier blocks AZ_i at the same flat index e, r0v = R0[row][c] - cx_gram_row on the long vector of length n * nrhs
template <typename C>
__device__ __forceinline__ void cx_gram_item(double* gs, const CxVecArgsT<C>& v, size_t e, C wv, C r0v) {
  const int j = v.gj;
  C azv[GRAM_MAXV - 1];
#pragma unroll
  for (int i = 0; i < GRAM_MAXV - 1; ++i) azv[i] = i < j ? v.az[(size_t)i * v.ldz + e] : C{};
  double s[GRAM_NS];
#pragma unroll
  for (int q = 0; q < GRAM_NS; ++q) s[q] = 0.0;
  cx_gram_row(s, j, azv, wv, r0v);
#pragma unroll
  for (int q = 0; q < GRAM_NS; ++q) gs[q] += s[q];
}

template <int MODE, typename PTR, typename VT, typename C>
__global__ __launch_bounds__(BLK) void cx_csr_stream_spmm(CxCsrDev<PTR, VT> A, CxVecArgsT<C> v, int nrhs, int lg) {
  __shared__ VT sval[CX_CHUNK];
  __shared__ int scol[CX_CHUNK];
  __shared__ int srow[MAXROWS + 1];
  __shared__ C lred[BLK];
  __shared__ double red[(MODE == GRAM ? GRAM_NS : 1) * (BLK / 64)];

  const int tid = threadIdx.x;
  const int G = 1 << lg;
  const int bid = xcd_band(blockIdx.x, A.nblocks);
  const int r0 = A.blk_row[bid];
  const int r1 = A.blk_row[bid + 1];
  const int nrows = r1 - r0;
  const PTR k0 = A.rowptr[r0];
  const PTR k1 = A.rowptr[r1];
  const int c = tid & (G - 1);

  if (nrows == 1 && (k1 - k0) > CX_CHUNK) {
    // one row longer than a chunk: lane group g takes the entries g, g + BLK / G, ...
    C acc = C{};
    if (c < nrhs)
      for (PTR k = k0 + (tid >> lg); k < k1; k += BLK >> lg) acc += cmul(A.val[k], v.x[(size_t)A.colidx[k] * nrhs + c]);
    lred[tid] = acc;
    __syncthreads();
    double sq = 0.0;
    double gs[MODE == GRAM ? GRAM_NS : 1];
#pragma unroll
    for (int q = 0; q < (MODE == GRAM ? GRAM_NS : 1); ++q) gs[q] = 0.0;
    if (tid < nrhs) {   // (tid == c: one lane per column, lane-group order)
      C s = C{};
      for (int g = 0; g < (BLK >> lg); ++g) s += lred[(g << lg) + tid];
      const size_t e = (size_t)r0 * nrhs + tid;
      C pb = C{}, pd = pb, px = pb;
      cx_operands_blk<MODE>(v, r0, e, pb, pd, px);
      const C o = cx_epilogue<MODE>(v, s, pb, pd, px);
      v.y[e] = o;
      sq = cabs2(o);
      if (MODE == RESID && v.z1) v.z1[e] = cmul(pd, o);
      if constexpr (MODE == GRAM) {
        if (v.znext) v.znext[e] = cmul(pd, o);
        cx_gram_item(gs, v, e, o, pb);
      }
    }
    if constexpr (MODE == GRAM) {   // the block's only row: the scalars of its nrhs result lanes, summed in the first wavefront
      if (tid < 64) {
        const int ns = 2 * v.gj + 3;
#pragma unroll
        for (int q = 0; q < GRAM_NS; ++q)
          if (q < ns) {   // (uniform)
            double t = gs[q];
            for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
            if (tid == 0) v.gpart[(size_t)q * A.nblocks + bid] = t;
          }
      }
      return;
    }
    if (v.sumsq && tid < 64) {   // nrhs <= 16: the columns sit in the first wavefront
      for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
      if (tid == 0) v.sumsq[bid] = sq;
    }
    return;
  }

  // ---- every global load of the matrix stream up front, staged in LDS ----------------------------
  VT va[CX_ITEMS];
  int ca[CX_ITEMS];
#pragma unroll
  for (int it = 0; it < CX_ITEMS; ++it) {
    const PTR idx = k0 + it * BLK + tid;
    if (idx < k1) {
      va[it] = A.val[idx];
      ca[it] = A.colidx[idx];
    } else {
      va[it] = VT{};
      ca[it] = 0;
    }
  }
  if (tid <= nrows) srow[tid] = (int)(A.rowptr[r0 + tid] - k0);
  if (tid == 0 && nrows == MAXROWS) srow[MAXROWS] = (int)(k1 - k0);
#pragma unroll
  for (int it = 0; it < CX_ITEMS; ++it) {
    sval[it * BLK + tid] = va[it];
    scol[it * BLK + tid] = ca[it];
  }
  __syncthreads();
  // ---- one lane per (row, column): the row from LDS in stored order, fused epilogue ---------------
  double sq = 0.0;
  double gs[MODE == GRAM ? GRAM_NS : 1];
#pragma unroll
  for (int q = 0; q < (MODE == GRAM ? GRAM_NS : 1); ++q) gs[q] = 0.0;
  const int nitems = nrows << lg;
  for (int t = tid; t < nitems; t += BLK) {
    const int lrow = t >> lg;
    if (c >= nrhs) continue;
    const int row = r0 + lrow;
    const size_t e = (size_t)row * nrhs + c;
    C pb = C{}, pd = pb, px = pb;
    cx_operands_blk<MODE>(v, row, e, pb, pd, px);
    C acc = C{};
    const int s = srow[lrow], en = srow[lrow + 1];
    for (int k = s; k < en; ++k) acc += cmul(sval[k], v.x[(size_t)scol[k] * nrhs + c]);
    const C o = cx_epilogue<MODE>(v, acc, pb, pd, px);
    v.y[e] = o;
    if (MODE == RESID && v.z1) v.z1[e] = cmul(pd, o);
    if constexpr (MODE == GRAM) {
      if (v.znext) v.znext[e] = cmul(pd, o);
      cx_gram_item(gs, v, e, o, pb);
    } else {
      sq += cabs2(o);
    }
  }
  if constexpr (MODE == GRAM) {
    // 2 j + 3 scalars over all rows AND columns of the row block: a lane's registers over the items it owns, wavefront shuffles, the
    // workgroup's LDS, one partial per scalar and row block - the vector form's slots, no atomics, the same bits on every run
    const int ns = 2 * v.gj + 3;
#pragma unroll
    for (int q = 0; q < GRAM_NS; ++q)
      if (q < ns) {   // (uniform)
        double t = gs[q];
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
        if ((tid & 63) == 0) red[q * (BLK / 64) + (tid >> 6)] = t;
      }
    __syncthreads();
    if (tid < ns) {
      double t = 0.0;
      for (int w = 0; w < BLK / 64; ++w) t += red[tid * (BLK / 64) + w];
      v.gpart[(size_t)tid * A.nblocks + bid] = t;
    }
    return;
  }
  if (v.sumsq) {   // a deterministic per-block partial of sum |out|^2 over all columns, summed by sum_final
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
    if ((tid & 63) == 0) red[tid >> 6] = sq;
    __syncthreads();
    if (tid == 0) {
      double t = 0.0;
      for (int w = 0; w < BLK / 64; ++w) t += red[w];
      v.sumsq[bid] = t;
    }
  }
}

// x[i][:] = d[i] * b[i][:] on a row-major block (the first sweep of relax from X = 0); m = n * nrhs
template <typename C>
__global__ __launch_bounds__(BLK) void cx_dscale_blk(const C* __restrict__ d, const C* __restrict__ b, C* __restrict__ x, long long m,
                                                     int nrhs) {
  const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
  if (i < m) x[i] = cmul(d[i / nrhs], b[i]);
}

// coarsest solve from the explicit inverse on a block: X = Ainv * B, B and X row-major [n][nrhs]; one wavefront per (row, column)
__global__ __launch_bounds__(BLK) void cx_dense_matblk(const d2_t* __restrict__ Ainv, const d2_t* __restrict__ b, d2_t* __restrict__ x,
                                                       int n, int nrhs) {
  const long long wave = ((long long)blockIdx.x * BLK + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= (long long)n * nrhs) return;   // wave-uniform
  const int row = (int)(wave / nrhs), c = (int)(wave - (long long)row * nrhs);
  const d2_t* a = Ainv + (size_t)row * n;
  d2_t acc = d2_t{0.0, 0.0};
  for (int j = lane; j < n; j += 64) acc += cmul(a[j], b[(size_t)j * nrhs + c]);
  for (int o = 32; o > 0; o >>= 1) acc += shfl_xor_v(acc, o);
  if (lane == 0) x[wave] = acc;
}

// The block helpers of the complex block Krylov driver (the complex forms of blk_gram_partial / blk_gram_final / blk_comb,
// mg_kernels.hpp): blocks row-major [n][k], k <= BLK_KMAX.
//   cx_blk_gram_partial / _final:  G = X^H Y (k x k), G[a][b] = sum_i conj(X[i][a]) Y[i][b]: deterministic two-stage reduction
//   cx_blk_comb:                   out[i,:] = s * add[i,:] + in[i,:] * Cm   (Cm k x k complex, row-major; out may alias in / add)
__global__ __launch_bounds__(BLK) void cx_blk_gram_partial(const d2_t* __restrict__ X, const d2_t* __restrict__ Y, long long n, int k,
                                                           d2_t* __restrict__ partial) {
  __shared__ d2_t red[BLK / 64][BLK_KMAX];
  const int a = blockIdx.y;
  d2_t acc[BLK_KMAX];
#pragma unroll
  for (int b = 0; b < BLK_KMAX; ++b) acc[b] = d2_t{0.0, 0.0};
  const long long stride = (long long)gridDim.x * BLK;
  for (long long i = (long long)blockIdx.x * BLK + threadIdx.x; i < n; i += stride) {
    const d2_t xa = X[i * k + a];
    const d2_t xc = d2_t{xa.x, -xa.y};
#pragma unroll
    for (int b = 0; b < BLK_KMAX; ++b)
      if (b < k) acc[b] += cmul(xc, Y[i * k + b]);
  }
#pragma unroll
  for (int b = 0; b < BLK_KMAX; ++b) {
    d2_t t = acc[b];
    for (int o = 32; o > 0; o >>= 1) t += shfl_xor_v(t, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][b] = t;
  }
  __syncthreads();
  if (threadIdx.x < k) {
    d2_t t = d2_t{0.0, 0.0};
    for (int w = 0; w < BLK / 64; ++w) t += red[w][threadIdx.x];
    partial[((size_t)blockIdx.x * k + a) * k + threadIdx.x] = t;
  }
}
__global__ __launch_bounds__(BLK) void cx_blk_gram_final(const d2_t* __restrict__ partial, int nb, int k, d2_t* __restrict__ out) {
  const int e = threadIdx.x;   // entry a*k + b
  if (e >= k * k) return;
  d2_t t = d2_t{0.0, 0.0};
  for (int p = 0; p < nb; ++p) t += partial[(size_t)p * k * k + e];
  out[e] = t;
}
__global__ __launch_bounds__(BLK) void cx_blk_comb(d2_t* out, const d2_t* add, d2_t s, const d2_t* in, const d2_t* __restrict__ Cm,
                                                   long long n, int k) {
  __shared__ d2_t sc[BLK_KMAX * BLK_KMAX];
  for (int t = threadIdx.x; t < k * k; t += BLK) sc[t] = Cm[t];
  __syncthreads();
  // one lane per row, as blk_comb: the whole row of `in` is in registers before the row of `out` is written (out may alias in)
  const long long stride = (long long)gridDim.x * BLK;
  for (long long i = (long long)blockIdx.x * BLK + threadIdx.x; i < n; i += stride) {
    d2_t row[BLK_KMAX], o[BLK_KMAX];
#pragma unroll
    for (int a = 0; a < BLK_KMAX; ++a) row[a] = a < k ? in[i * k + a] : d2_t{0.0, 0.0};
#pragma unroll
    for (int b = 0; b < BLK_KMAX; ++b) o[b] = (b < k && add) ? cmul(s, add[i * k + b]) : d2_t{0.0, 0.0};
#pragma unroll
    for (int a = 0; a < BLK_KMAX; ++a)
      if (a < k) {
#pragma unroll
        for (int b = 0; b < BLK_KMAX; ++b)
          if (b < k) o[b] += cmul(row[a], sc[a * k + b]);
      }
#pragma unroll
    for (int b = 0; b < BLK_KMAX; ++b)
      if (b < k) out[i * k + b] = o[b];
  }
}

// The Gram kernels of the complex block FGMRES driver (mg_complex_krylov.inc: cx_block_fgmres_dev), which needs j + 3 Gram matrices
// per inner step j.  cx_blk_gram_partial above runs k workgroup rows that each stream the whole of Y again; these read every
// element of X and of Y from HBM ONCE (X == Y: once in all).
//   cx_blk_gram_onepass:  G = X^H Y.  A workgroup stages a tile of GRAM_TILE / kk rows of X and of Y in LDS (kk = pow2 >= k; a tile is
//     one contiguous run of at most GRAM_TILE entries, 16 KiB per operand, loaded coalesced and prefetched into registers one tile
//     ahead).  The BLK lanes form BLK / kk^2 groups of kk^2 lanes; lane e of a group owns entry (a, b) = (e / kk, e % kk) and sums
//     it over the tile rows r = group, group + groups, ... in ONE register: a lane holds one accumulator, never k^2.  The reads of
//     sx[r][a] are a broadcast over kk lanes, those of sy[r][b] kk consecutive 16-byte words.  At the end the groups are added in
//     group order through LDS and the workgroup writes one k x k partial; cx_blk_gram_final_wave adds the partials, one wavefront
//     per entry.  Every entry is a sum in a fixed order: rows of a lane in order, groups in order, workgroups in the final kernel's
//     fixed order - no atomics.
//   cx_blk_comb_gram:  cx_blk_comb (the same operations in the same order, so the same bits in `out`) with an epilogue that leaves
//     the partials of G = Q^H out, Q == out or a block that overlaps none of the others: every lane puts the row of `out` it has just
//     written (from its registers) and its row of Q into the staged tile, GRAM_TILE / kk rows per round, and the workgroup sums the
//     tile as above.  `out` is not read again from HBM.
constexpr int GRAM_TILE = 1024;
struct GramLane {
  int a, b, g, groups;
  bool on;
  __device__ __forceinline__ GramLane(int k, int lgk) {
    const int e = threadIdx.x & ((1 << (2 * lgk)) - 1);
    a = e >> lgk;
    b = e & ((1 << lgk) - 1);
    g = threadIdx.x >> (2 * lgk);
    groups = BLK >> (2 * lgk);
    on = a < k && b < k;
  }
};
__device__ __forceinline__ void cx_gram_tile(const d2_t* sx, const d2_t* sy, int rows, int k, const GramLane& L, d2_t& acc) {
  if (!L.on) return;
  for (int r = L.g; r < rows; r += L.groups) {
    const d2_t xa = sx[r * k + L.a];
    acc += cmul(d2_t{xa.x, -xa.y}, sy[r * k + L.b]);
  }
}
__device__ __forceinline__ void cx_gram_store(d2_t* red, d2_t acc, int k, const GramLane& L, d2_t* __restrict__ partial) {
  red[threadIdx.x] = acc;
  __syncthreads();
  if (L.g == 0 && L.on) {
    const int kk2 = BLK / L.groups;
    d2_t t = d2_t{0.0, 0.0};
    for (int g = 0; g < L.groups; ++g) t += red[g * kk2 + threadIdx.x];
    partial[(size_t)blockIdx.x * k * k + L.a * k + L.b] = t;
  }
}
// the partials of nb workgroups added per entry by ONE WAVEFRONT (grid: k * k workgroups of 64 lanes): lane l adds the partials
// l, l + 64, ... in that order, the 64 lane sums are added by a fixed butterfly - a fixed order again, and a few microseconds where
// the one lane per entry of cx_blk_gram_final walks the partials one load latency at a time
__global__ __launch_bounds__(64) void cx_blk_gram_final_wave(const d2_t* __restrict__ partial, int nb, int k, d2_t* __restrict__ out) {
  const int e = blockIdx.x;   // entry a*k + b
  d2_t t = d2_t{0.0, 0.0};
  for (int p = threadIdx.x; p < nb; p += 64) t += partial[(size_t)p * k * k + e];
  for (int o = 32; o > 0; o >>= 1) t += shfl_xor_v(t, o);
  if (threadIdx.x == 0) out[e] = t;
}
__global__ __launch_bounds__(BLK) void cx_blk_gram_onepass(const d2_t* X, const d2_t* Y, long long n, int k, int lgk, d2_t* __restrict__ partial) {
  __shared__ d2_t sx[GRAM_TILE], sy[GRAM_TILE], red[BLK];
  constexpr int PER = GRAM_TILE / BLK;
  const int tid = threadIdx.x;
  const GramLane L(k, lgk);
  const bool same = X == Y;
  const int tr = GRAM_TILE >> lgk;                 // rows of a tile
  const int tlen = tr * k;                         // its entries (<= GRAM_TILE)
  const long long ntiles = (n + tr - 1) / tr, total = n * k;
  d2_t px[PER], py[PER];
  long long tile = blockIdx.x;
#pragma unroll
  for (int it = 0; it < PER; ++it) {
    const int l = it * BLK + tid;
    const long long idx = tile * tlen + l;
    const bool ok = tile < ntiles && l < tlen && idx < total;
    px[it] = ok ? X[idx] : d2_t{0.0, 0.0};
    py[it] = (ok && !same) ? Y[idx] : d2_t{0.0, 0.0};
  }
  d2_t acc = d2_t{0.0, 0.0};
  for (; tile < ntiles; tile += gridDim.x) {
#pragma unroll
    for (int it = 0; it < PER; ++it) {
      sx[it * BLK + tid] = px[it];
      if (!same) sy[it * BLK + tid] = py[it];
    }
    __syncthreads();
    const long long next = tile + gridDim.x;       // the next tile's loads are in flight while this one is summed
#pragma unroll
    for (int it = 0; it < PER; ++it) {
      const int l = it * BLK + tid;
      const long long idx = next * tlen + l;
      const bool ok = next < ntiles && l < tlen && idx < total;
      px[it] = ok ? X[idx] : d2_t{0.0, 0.0};
      py[it] = (ok && !same) ? Y[idx] : d2_t{0.0, 0.0};
    }
    const int rows = (int)((n - tile * tr) < (long long)tr ? (n - tile * tr) : (long long)tr);
    cx_gram_tile(sx, same ? sx : sy, rows, k, L, acc);
    __syncthreads();
  }
  cx_gram_store(red, acc, k, L, partial);
}
__global__ __launch_bounds__(BLK) void cx_blk_comb_gram(d2_t* out, const d2_t* add, d2_t s, const d2_t* in, const d2_t* __restrict__ Cm,
                                                        const d2_t* Q, long long n, int k, int lgk, d2_t* __restrict__ partial) {
  __shared__ d2_t sc[BLK_KMAX * BLK_KMAX];
  __shared__ d2_t sx[GRAM_TILE], sy[GRAM_TILE], red[BLK];
  const int tid = threadIdx.x;
  for (int t = tid; t < k * k; t += BLK) sc[t] = Cm[t];
  __syncthreads();
  const GramLane L(k, lgk);
  const bool self = Q == out;
  const int rpr = (GRAM_TILE >> lgk) < BLK ? (GRAM_TILE >> lgk) : BLK;   // rows of a round
  d2_t acc = d2_t{0.0, 0.0};
  const long long stride = (long long)gridDim.x * BLK;
  for (long long base = (long long)blockIdx.x * BLK; base < n; base += stride) {   // (uniform over the workgroup)
    const long long i = base + tid;
    const bool live = i < n;
    d2_t row[BLK_KMAX], o[BLK_KMAX];
    if (live) {
#pragma unroll
      for (int a = 0; a < BLK_KMAX; ++a) row[a] = a < k ? in[i * k + a] : d2_t{0.0, 0.0};
#pragma unroll
      for (int b = 0; b < BLK_KMAX; ++b) o[b] = (b < k && add) ? cmul(s, add[i * k + b]) : d2_t{0.0, 0.0};
#pragma unroll
      for (int a = 0; a < BLK_KMAX; ++a)
        if (a < k) {
#pragma unroll
          for (int b = 0; b < BLK_KMAX; ++b)
            if (b < k) o[b] += cmul(row[a], sc[a * k + b]);
        }
#pragma unroll
      for (int b = 0; b < BLK_KMAX; ++b)
        if (b < k) out[i * k + b] = o[b];
    }
    const int here = (int)((n - base) < (long long)BLK ? (n - base) : (long long)BLK);   // rows of this trip
    for (int r0 = 0; r0 < here; r0 += rpr) {
      if (live && tid >= r0 && tid < r0 + rpr) {
        const int lr = tid - r0;
#pragma unroll
        for (int b = 0; b < BLK_KMAX; ++b)
          if (b < k) {
            sy[lr * k + b] = o[b];
            if (!self) sx[lr * k + b] = Q[i * k + b];
          }
      }
      __syncthreads();
      cx_gram_tile(self ? sy : sx, sy, (here - r0) < rpr ? (here - r0) : rpr, k, L, acc);
      __syncthreads();
    }
  }
  cx_gram_store(red, acc, k, L, partial);
}

// x = d.*b: relax's only update when the sweep starts from x = 0 (MGcycle.jl:134 with r = b)
template <typename C>
__global__ __launch_bounds__(BLK) void cx_dscale(const C* __restrict__ d, const C* __restrict__ b, C* __restrict__ x, long long n) {
  const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
  if (i < n) x[i] = cmul(d[i], b[i]);
}

// first pass of the deterministic sum of |z_i|^2: one partial per workgroup (second pass: sum_final)
template <typename C>
__global__ __launch_bounds__(BLK) void cx_sumsq_partial(const C* __restrict__ z, long long n, double* __restrict__ partial) {
  __shared__ double red[BLK / 64];
  const long long stride = (long long)gridDim.x * BLK;
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * BLK + threadIdx.x; i < n; i += stride) acc += cabs2(z[i]);
  const double s = block_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// z = d.*b with the partials of sum |b_i|^2, one per workgroup: the front of an FGMRES relaxation from x = 0 (r0 = b; z_1 = MM(r0),
// rnorm0 = norm(r0), FGMRES.jl:65,84).  Grid-stride, so any grid covers n; the host launches one workgroup per row block of the
// level's operator, which is the stride of the relaxation's partial sums.
// (C = f2_t: the product in single, the partials in double all the same.)
template <typename C>
__global__ __launch_bounds__(BLK) void cx_dscale_sumsq(const C* __restrict__ d, const C* __restrict__ b, C* __restrict__ z, long long n,
                                                       double* __restrict__ partial) {
  __shared__ double red[BLK / 64];
  const long long stride = (long long)gridDim.x * BLK;
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * BLK + threadIdx.x; i < n; i += stride) {
    const C bv = b[i];
    z[i] = cmul(d[i], bv);
    acc += cabs2(bv);
  }
  const double s = block_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// The same front for a row-major block [n][nrhs] (m = n * nrhs): Z_1 = d.*B with d[row] shared by the columns, and the partials of
// ||B||_F^2 - the long vector's rnorm0 (FGMRES.jl:51-53, 65)
template <typename C>
__global__ __launch_bounds__(BLK) void cx_dscale_sumsq_blk(const C* __restrict__ d, const C* __restrict__ b, C* __restrict__ z, long long m,
                                                           int nrhs, double* __restrict__ partial) {
  __shared__ double red[BLK / 64];
  const long long stride = (long long)gridDim.x * BLK;
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * BLK + threadIdx.x; i < m; i += stride) {
    const C bv = b[i];
    z[i] = cmul(d[i / nrhs], bv);
    acc += cabs2(bv);
  }
  const double s = block_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// The two conversion passes of the mixed-precision preconditioner (SolveFuncs.jl:52-58: bl .= b ... z2 .= z), one element per
// lane: the ComplexF64 side is one 16-byte access, the ComplexF32 side one 8-byte access.
__global__ __launch_bounds__(BLK) void cx_narrow(const d2_t* __restrict__ src, f2_t* __restrict__ dst, long long n) {
  const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
  if (i < n) {
    const d2_t a = src[i];
    dst[i] = f2_t{(float)a.x, (float)a.y};
  }
}
__global__ __launch_bounds__(BLK) void cx_widen(const f2_t* __restrict__ src, d2_t* __restrict__ dst, long long n) {
  const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
  if (i < n) {
    const f2_t a = src[i];
    dst[i] = d2_t{(double)a.x, (double)a.y};
  }
}

// coarsest solve from the explicit inverse: x = Ainv * b, Ainv row-major n x n complex; one wavefront per row
__global__ __launch_bounds__(BLK) void cx_dense_matvec(const d2_t* __restrict__ Ainv, const d2_t* __restrict__ b,
                                                       d2_t* __restrict__ x, int n) {
  const long long wave = ((long long)blockIdx.x * BLK + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= n) return;
  const d2_t* a = Ainv + wave * (long long)n;
  d2_t acc = d2_t{0.0, 0.0};
  for (int j = lane; j < n; j += 64) acc += cmul(a[j], b[j]);
  for (int o = 32; o > 0; o >>= 1) acc += shfl_xor_v(acc, o);
  if (lane == 0) x[wave] = acc;
}

// ------------------------------------------------------------------------------------------------
// replaceMatrixInHierarchy on a CF64 hierarchy (mg_rap_CF64; MGsetup.jl:226-270): the numeric Galerkin product on C's fixed
// pattern and getRelaxPrec for complex values.  Device A holds the APPLIED values (conjugated once at upload) and R, P are
// real, so C = R*(A*P) needs no conjugation anywhere.
//
// cx_rap_numeric: the walk of rap_numeric (mg_kernels.hpp) with complex sums and with `groups` rows of A side by side.  One
// wavefront per coarse row i.  The entries (i,k) of R's row are walked one after the other in stored order.  The wavefront is
// cut into `groups` lane groups of 64/groups lanes: group g takes the entries (k,j) of A's row number g, g + groups, ... in
// stored order, and spreads the entries (j,c) of ONE row of P - distinct target columns - over its lanes; each lane finds its
// column in C's sorted row by binary search in LDS and adds into ITS GROUP'S copy of the accumulator, without atomics.  The
// copies are summed in group order at the end.  Every entry of C is therefore the same sum in the same order on every run
// of one configuration (groups = 1 is rap_numeric's order exactly; another group count is another, equally fixed order).  On a GMG level a row of P holds at most 8 entries: one group of 64 lanes
// leaves 56 idle, 8 groups of 8 walk 8 rows of A at once.
// The accumulator is dynamic LDS, (16 * groups + 4) bytes per target column, sized by the host to min(rap_chunk, the level's
// longest row of C) columns - 3.6 KB on a GMG level (27-entry rows, 8 groups), where a fixed RAP_CAP of complex sums would
// take 40 KB per wavefront; longer rows are accumulated `chunk` target columns at a time by the same walk.  Rows of R, A, P
// and C may be empty.
// ------------------------------------------------------------------------------------------------
constexpr int CX_RAP_GROUPS = 8;   // lane groups of cx_rap_numeric unless the option rap_groups says otherwise
template <typename VT>
struct CxCsr32 {
  const int* rowptr;
  const int* colidx;
  const VT* val;
};

// The stored value types are template arguments: AV the pairs of A and C (d2_t, or f2_t on a CF32 handle), TV the scalars of R and P
// (double or float).  A single value is widened as it is loaded (cx_wide: exact), every product and sum is the ComplexF64 one - the
// same walk, lane groups, LDS accumulator of d2_t and summation order for both - and the result is rounded once, where it is stored
// (cx_store_as).  For d2_t / double both helpers are the identity: the ComplexF64 instantiation is the code it was.
__device__ __forceinline__ d2_t cx_wide(d2_t a) { return a; }
__device__ __forceinline__ d2_t cx_wide(f2_t a) { return d2_t{(double)a.x, (double)a.y}; }
__device__ __forceinline__ void cx_store_as(d2_t* p, d2_t a) { *p = a; }
__device__ __forceinline__ void cx_store_as(f2_t* p, d2_t a) { *p = f2_t{(float)a.x, (float)a.y}; }

template <typename AV, typename TV>
__global__ __launch_bounds__(64) void cx_rap_numeric(CxCsr32<TV> R, CxCsr32<AV> A, CxCsr32<TV> P,
                                                     const int* __restrict__ Crowptr, const int* __restrict__ Ccol,
                                                     AV* __restrict__ Cval, int chunk, int groups) {
  extern __shared__ d2_t cx_rap_lds[];   // groups copies of chunk sums, then chunk column indices
  d2_t* sacc = cx_rap_lds;
  int* scol = reinterpret_cast<int*>(cx_rap_lds + (size_t)groups * chunk);
  const int i = blockIdx.x;
  const int lane = threadIdx.x;
  const int W = 64 / groups;             // lanes per group (groups is a power of two <= 64: host)
  const int g = lane / W, sub = lane - g * W;
  d2_t* mine = sacc + (size_t)g * chunk;
  const int c0 = Crowptr[i];
  const int len = Crowptr[i + 1] - c0;
  for (int t0 = 0; t0 < len; t0 += chunk) {
    const int clen = len - t0 < chunk ? len - t0 : chunk;
    __syncthreads();
    for (int t = lane; t < clen; t += 64) scol[t] = Ccol[c0 + t0 + t];
    for (int t = lane; t < groups * chunk; t += 64) sacc[t] = d2_t{0.0, 0.0};
    __syncthreads();
    const int cmin = scol[0], cmax = scol[clen - 1];
    for (int kk = R.rowptr[i]; kk < R.rowptr[i + 1]; ++kk) {        // wave-uniform, stored order
      const int k = R.colidx[kk];
      const double rv = (double)R.val[kk];
      const int a1 = A.rowptr[k + 1];
      for (int jj0 = A.rowptr[k]; jj0 < a1; jj0 += groups) {        // wave-uniform; group g: entry jj0 + g
        const int jj = jj0 + g;
        if (jj < a1) {
          const int j = A.colidx[jj];
          const d2_t ra = cmul(rv, cx_wide(A.val[jj]));
          for (int pp = P.rowptr[j] + sub; pp < P.rowptr[j + 1]; pp += W) {   // distinct columns: one lane each
            const int c = P.colidx[pp];
            if (c < cmin || c > cmax) continue;                     // (another chunk's column)
            int lo = 0, hi = clen - 1;
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (scol[mid] < c) lo = mid + 1;
              else hi = mid;
            }
            if (scol[lo] == c) mine[lo] += cmul((double)P.val[pp], ra);
          }
        }
        __builtin_amdgcn_wave_barrier();   // one wavefront: LDS accesses of the next rows of P follow in program order
      }
    }
    __syncthreads();
    for (int t = lane; t < clen; t += 64) {
      d2_t s = sacc[t];
      for (int q = 1; q < groups; ++q) s += sacc[(size_t)q * chunk + t];   // group order
      cx_store_as(Cval + c0 + t0 + t, s);
    }
  }
}

// z_k = conj(z_k) in place: the reference's AT values <-> the applied values the kernels hold
__global__ __launch_bounds__(BLK) void cx_conj(d2_t* __restrict__ z, long long n) {
  const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
  if (i < n) z[i].y = -z[i].y;
}

template <typename AV>
__device__ __forceinline__ d2_t cx_diag(const CxCsr32<AV>& A, int i) {
  d2_t diag = d2_t{0.0, 0.0};
  for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k)
    if (A.colidx[k] == i) diag = cx_wide(A.val[k]);
  return diag;
}
// d_i = omega / a_ii  (getRelaxPrec "Jac" for complex values: conj(relaxParam ./ diag(AT)), MGsetup.jl:145-147)
// (AV: A's stored pairs, DV: d's - the GMRES coarsest vector of a CF32 handle is ComplexF64 from the widened operator)
// cdiv((omega, 0), a) with contraction off, so that the vector is one fixed sequence of roundings (as cx_colsumsq's sums are):
// s = fl(fl(x x) + fl(y y)), d = (fl(fl(omega x) + fl(0 y)) / s, fl(fl(0 x) - fl(omega y)) / s).
__device__ __forceinline__ d2_t cx_jac_div(double omega, d2_t a) {
#pragma clang fp contract(off)
  const double xx = a.x * a.x;
  const double yy = a.y * a.y;
  const double s = xx + yy;
  const double ox = omega * a.x;
  const double zy = 0.0 * a.y;
  const double zx = 0.0 * a.x;
  const double oy = omega * a.y;
  const double nr = ox + zy;
  const double ni = zx - oy;
  return d2_t{nr / s, ni / s};
}
template <typename AV, typename DV>
__global__ __launch_bounds__(BLK) void cx_relax_jacobi(CxCsr32<AV> A, int n, double omega, DV* __restrict__ d) {
  const int i = blockIdx.x * BLK + threadIdx.x;
  if (i >= n) return;
  cx_store_as(d + i, cx_jac_div(omega, cx_diag(A, i)));
}
// s_j = sum over the entries of COLUMN j of re^2 + im^2 in ascending row order (getSPAIprec, MGsetup.jl:359-362: row j of AT):
// squares rounded, then summed, as colsumsq_kernel does - no atomics, the same bits on every run and as the host's bincount.
template <typename AV>
__global__ __launch_bounds__(BLK) void cx_colsumsq(const AV* __restrict__ val, const int* __restrict__ tptr,
                                                   const int* __restrict__ tperm, int n_cols, double* __restrict__ s) {
#pragma clang fp contract(off)
  const int j = blockIdx.x * BLK + threadIdx.x;
  if (j >= n_cols) return;
  double acc = 0.0;
  for (int k = tptr[j]; k < tptr[j + 1]; ++k) {
    const d2_t a = cx_wide(val[tperm[k]]);
    const double re2 = a.x * a.x;
    const double im2 = a.y * a.y;
    const double sq = re2 + im2;
    acc = acc + sq;
  }
  s[j] = acc;
}
// d_i = omega * conj(a_ii) / s_i  (conj(relaxParam * getSPAIprec(AT)), MGsetup.jl:148-149): the quotient first
template <typename AV>
__global__ __launch_bounds__(BLK) void cx_relax_spai(CxCsr32<AV> A, int n, double omega, const double* __restrict__ s,
                                                     AV* __restrict__ d) {
  const int i = blockIdx.x * BLK + threadIdx.x;
  if (i >= n) return;
  const d2_t diag = cx_diag(A, i);
  const double si = s[i];
  cx_store_as(d + i, d2_t{omega * (diag.x / si), omega * (-diag.y / si)});
}

// ------------------------------------------------------------------------------------------------
// adjointHierarchy on a complex hierarchy (mg_adjoint_hierarchy_CF64 / _CF32; MGsetup.jl:274-318 for complex VAL): the stored-order
// CSR of M' = conj(M)^T built in HBM from M's CSR; neither the values nor the column indices travel to the host.
//   cx_adj_count    one lane per entry: cnt[col] += 1 (integer atomics: exact, any order)
//   (host)          the n_cols counts come back (4 B per column), are scanned into the new row pointers and cut into row blocks
//   cx_adj_scatter  one lane per entry (row i, column c): its row index into a free slot of column c's segment (an atomic cursor
//                   per column hands out the slots: any order)
//   cx_adj_order    one lane per entry again: the entry's place in its segment is the number of entries of that segment with a
//                   smaller row index (the rows of one column are distinct), so lane k writes (i, conj(val_k)) to tptr[c] + rank -
//                   the same place whatever order the scatter left, the same bits on every run, what a host transpose gives.
// The row of entry k is found by bisection in rowptr (rows may be empty).  The ranking reads a segment once per entry of it: the
// work is the sum of the squared column lengths (27^2 per column on a GMG level), the host refuses columns beyond 4096 entries.
// Values: complex pairs are conjugated on the way (A), real ones copied (R -> P).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ d2_t cx_adj_val(d2_t a) { return d2_t{a.x, -a.y}; }
__device__ __forceinline__ f2_t cx_adj_val(f2_t a) { return f2_t{a.x, -a.y}; }
__device__ __forceinline__ double cx_adj_val(double a) { return a; }
__device__ __forceinline__ float cx_adj_val(float a) { return a; }

// the row that holds entry k: the last i with rowptr[i] <= k (0 <= k < rowptr[n_rows])
__device__ __forceinline__ int cx_row_of(const int* __restrict__ rowptr, int n_rows, int k) {
  int lo = 0, hi = n_rows;   // the first index whose pointer exceeds k lies in (0, n_rows]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (rowptr[mid] <= k) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}

__global__ __launch_bounds__(BLK) void cx_adj_count(const int* __restrict__ col, int nnz, int* __restrict__ cnt) {
  const long long k = (long long)blockIdx.x * BLK + threadIdx.x;
  if (k < nnz) atomicAdd(cnt + col[k], 1);
}

__global__ __launch_bounds__(BLK) void cx_adj_scatter(const int* __restrict__ rowptr, const int* __restrict__ col, int n_rows, int nnz,
                                                      const int* __restrict__ tptr, int* __restrict__ cursor, int* __restrict__ trow) {
  const long long k = (long long)blockIdx.x * BLK + threadIdx.x;
  if (k >= nnz) return;
  const int c = col[k];
  trow[tptr[c] + atomicAdd(cursor + c, 1)] = cx_row_of(rowptr, n_rows, (int)k);
}

template <typename VT>
__global__ __launch_bounds__(BLK) void cx_adj_order(const int* __restrict__ rowptr, const int* __restrict__ col, const VT* __restrict__ val,
                                                    int n_rows, int nnz, const int* __restrict__ tptr, const int* __restrict__ trow,
                                                    int* __restrict__ ocol, VT* __restrict__ oval) {
  const long long k = (long long)blockIdx.x * BLK + threadIdx.x;
  if (k >= nnz) return;
  const int i = cx_row_of(rowptr, n_rows, (int)k);
  const int c = col[k];
  const int k0 = tptr[c], k1 = tptr[c + 1];
  int rank = 0;
  for (int q = k0; q < k1; ++q) rank += trow[q] < i ? 1 : 0;
  ocol[k0 + rank] = i;
  oval[k0 + rank] = cx_adj_val(val[k]);
}

// Ainv <- Ainv' in place (row-major n x n complex): (A')^-1 = (A^-1)', the complex twin of dense_transpose_inplace
__global__ __launch_bounds__(BLK) void cx_dense_adjoint_inplace(d2_t* __restrict__ a, int n) {
  const long long idx = (long long)blockIdx.x * BLK + threadIdx.x;
  const long long i = idx / n, j = idx - i * n;
  if (i >= n || j > i) return;
  const d2_t lo = a[i * n + j];
  if (j == i) {
    a[i * n + i] = cx_adj_val(lo);
  } else {
    a[i * n + j] = cx_adj_val(a[j * n + i]);
    a[j * n + i] = cx_adj_val(lo);
  }
}

// z_k = conj(z_k) in place on float pairs (relaxPrecs of a CF32 handle)
__global__ __launch_bounds__(BLK) void cx_conj32(f2_t* __restrict__ z, long long n) {
  const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
  if (i < n) z[i].y = -z[i].y;
}

// ------------------------------------------------------------------------------------------------
// Complex hybrid Kaczmarz relaxation (reference native: deps/src/parRelax.h:7-43 built with spValType = double complex,
// applyHybridKaczmarz_CFP64_INT64).  The schedule of the real hybrid_kaczmarz (mg_kernels.hpp): one wavefront per
// sub-domain, or one wavefront for all sub-domains in order when `sequential` is set; rows in list order, zero padding
// skipped, an nrhs loop over column-major blocks.  val is the reference's valA (nzval of the CSC of A^H = conj of A's CSR
// values) and invD is complex; for row i
//   inner = b_i - sum_k conj(val_k) x_k   (products in stored order, real and imaginary parts subtracted separately)
//   inner = inner * invD_i ;  x_k += inner * val_k  for every k of the row.
// Every product and sum is rounded separately with C99's plain formula (a+bi)(c+di) = (ac-bd) + (ad+bc)i, so the
// sequential schedule equals the reference binary run with one thread bit for bit.  The helpers below carry their own
// contract(off): the shared cmul above may be fused into FMAs.  x is read and written through L2 as two relaxed
// agent-scope 8-byte atomics per value (L1 bypassed): a row sees the rows before it, and other sub-domains see what they
// happen to see.  Racing sub-domains may read a value whose real and imaginary parts come from different updates (a torn
// pair); the reference's OpenMP threads race on the same nodes the same way, unsynchronised.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ d2_t kz_cmul(double ar, double ai, double br, double bi) {
#pragma clang fp contract(off)
  return d2_t{ar * br - ai * bi, ar * bi + ai * br};
}
__device__ __forceinline__ double kz_load(double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void kz_store(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(64) void hybrid_kaczmarz_c(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                        const d2_t* __restrict__ val, const unsigned int* __restrict__ arr,
                                                        int num_domains, int domain_length, double* x,
                                                        const double* __restrict__ b, int nrhs, long long n,
                                                        const d2_t* __restrict__ invD, int sequential) {
#pragma clang fp contract(off)   // every product and sum rounded separately, as in the reference's plain C (no FMA)
  const int lane = threadIdx.x;
  const int d0 = sequential ? 0 : blockIdx.x, d1 = sequential ? num_domains : blockIdx.x + 1;
  for (int dom = d0; dom < d1; ++dom) {
    for (int i = 0; i < domain_length; ++i) {
      const unsigned int row1 = arr[(size_t)dom * domain_length + i];
      if (row1 == 0) continue;   // zero padding (wave-uniform)
      const int row = (int)row1 - 1;
      const int s = rowptr[row], e = rowptr[row + 1];
      const d2_t di = invD[row];
      for (int c = 0; c < nrhs; ++c) {
        double* xc = x + (size_t)c * 2 * n;            // interleaved (re, im)
        const double* bc = b + (size_t)c * 2 * n;
        double ir = bc[2 * (size_t)row], ii = bc[2 * (size_t)row + 1];
        for (int k0 = s; k0 < e; k0 += 64) {
          const int k = k0 + lane;
          d2_t prod = d2_t{0.0, 0.0};
          if (k < e) {
            const d2_t v = val[k];
            double* xp = xc + 2 * (size_t)col[k];
            prod = kz_cmul(v.x, -v.y, kz_load(xp), kz_load(xp + 1));   // conj(val_k) * x_k
          }
          const int cnt = min(64, e - k0);
          for (int t = 0; t < cnt; ++t) {   // stored order
            ir = ir - __shfl(prod.x, t);
            ii = ii - __shfl(prod.y, t);
          }
        }
        const d2_t inner = kz_cmul(ir, ii, di.x, di.y);
        for (int k = s + lane; k < e; k += 64) {
          const d2_t v = val[k];
          double* xp = xc + 2 * (size_t)col[k];
          const double oldr = kz_load(xp), oldi = kz_load(xp + 1);
          const d2_t upd = kz_cmul(inner.x, inner.y, v.x, v.y);
          kz_store(xp, oldr + upd.x);
          kz_store(xp + 1, oldi + upd.y);
        }
        // the next row of this wavefront must see these stores: wait until L2 has acknowledged them
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Single hybrid Kaczmarz relaxation (applyHybridKaczmarz_FP32_INT64 / _CFP32_INT64: deps/src/parRelax.h:7-43 built with
// spValType = float / float complex), written once over the STORED type S = float or f2_t.  The schedule is that of
// hybrid_kaczmarz_c above.  The arithmetic mixes precisions per statement, because the reference's does: parRelax.h:27
// calls conj(), the DOUBLE complex function of <complex.h>, so in the single builds
//   inner -= conj(val_k) * x_k   widens val_k and x_k to double, forms the product in double (real: exact; complex: the plain
//                                formula, each part's sum rounded once to double), subtracts it from the widened inner in
//                                double and rounds inner back to single AFTER EVERY TERM (per part for complex);
//   inner *= invD_i ;  x_k += inner * val_k   stay in single: the plain complex formula, every product and sum rounded to float.
// The lanes form the double products in parallel; the subtraction chain runs over the shuffled products in stored order with
// the rounding to single after each term, so the sequential schedule equals the reference binary run with one thread bit for
// bit.  x is read and written through L2 with relaxed agent-scope atomics (L1 bypassed), one access per value: 4 bytes for
// float and ONE 8-byte access for a ComplexF32 pair, so - unlike the ComplexF64 kernel's two 8-byte halves - a pair read by a
// racing sub-domain always comes whole from one update (it cannot tear).  x must be aligned to sizeof(S).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float kzs_load(float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ f2_t kzs_load(f2_t* p) {
  const unsigned long long u = __hip_atomic_load(reinterpret_cast<unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return __builtin_bit_cast(f2_t, u);
}
__device__ __forceinline__ void kzs_store(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void kzs_store(f2_t* p, f2_t v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), __builtin_bit_cast(unsigned long long, v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
// conj(val) * x in double on the widened operands
__device__ __forceinline__ double kzs_prod(float v, float x) {
#pragma clang fp contract(off)
  return (double)v * (double)x;
}
__device__ __forceinline__ d2_t kzs_prod(f2_t v, f2_t x) { return kz_cmul((double)v.x, -(double)v.y, (double)x.x, (double)x.y); }
// inner = (S)((double)inner - lane t's product)
__device__ __forceinline__ float kzs_sub(float inner, double prod, int t) {
#pragma clang fp contract(off)
  return (float)((double)inner - __shfl(prod, t));
}
__device__ __forceinline__ f2_t kzs_sub(f2_t inner, d2_t prod, int t) {
#pragma clang fp contract(off)
  return f2_t{(float)((double)inner.x - __shfl(prod.x, t)), (float)((double)inner.y - __shfl(prod.y, t))};
}
// the single product: every operation rounded to float
__device__ __forceinline__ float kzs_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ f2_t kzs_mul(f2_t a, f2_t b) {
#pragma clang fp contract(off)
  return f2_t{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x};
}

template <typename S>
__global__ __launch_bounds__(64) void hybrid_kaczmarz_s(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                        const S* __restrict__ val, const unsigned int* __restrict__ arr,
                                                        int num_domains, int domain_length, S* x, const S* __restrict__ b,
                                                        int nrhs, long long n, const S* __restrict__ invD, int sequential) {
#pragma clang fp contract(off)   // every product and sum rounded separately, as in the reference's plain C (no FMA)
  const int lane = threadIdx.x;
  const int d0 = sequential ? 0 : blockIdx.x, d1 = sequential ? num_domains : blockIdx.x + 1;
  for (int dom = d0; dom < d1; ++dom) {
    for (int i = 0; i < domain_length; ++i) {
      const unsigned int row1 = arr[(size_t)dom * domain_length + i];
      if (row1 == 0) continue;   // zero padding (wave-uniform)
      const int row = (int)row1 - 1;
      const int s = rowptr[row], e = rowptr[row + 1];
      const S di = invD[row];
      for (int c = 0; c < nrhs; ++c) {
        S* xc = x + (size_t)c * n;
        S inner = b[(size_t)c * n + row];
        for (int k0 = s; k0 < e; k0 += 64) {
          const int k = k0 + lane;
          decltype(kzs_prod(S{}, S{})) prod{};
          if (k < e) prod = kzs_prod(val[k], kzs_load(xc + col[k]));
          const int cnt = min(64, e - k0);
          for (int t = 0; t < cnt; ++t) inner = kzs_sub(inner, prod, t);   // stored order, rounded to single after every term
        }
        inner = kzs_mul(inner, di);
        for (int k = s + lane; k < e; k += 64) {
          S* xp = xc + col[k];
          const S old = kzs_load(xp);
          const S upd = kzs_mul(inner, val[k]);
          kzs_store(xp, old + upd);
        }
        // the next row of this wavefront must see these stores: wait until L2 has acknowledged them
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Chip-wide sparse triangular solve of the factor applier (mg_lu_*_CFP64 / _CFP32 / _FP32): the form of sptrsv_level /
// sptrsv_tail_rhs / sptrsv_scatter / tri_gather_block / tri_inverse / tri_apply (mg_kernels.hpp), same layout and
// scheduling - one wavefront per row, one launch per wide level, up to 4 right-hand-side columns travelling together,
// the trailing chain of single-row levels replaced by the explicit inverse of its dense block, vectors row-major
// [n][nrhs], no inter-workgroup waiting.  Written once over the STORED value type S: d2_t (ComplexF64), f2_t (ComplexF32)
// or float, with the accumulation type lu_acc<S> of the single-workgroup sweep (mg_kernels.hpp): a single factor value and
// the gathered y are widened on load, the lane sums, the shuffles, the subtraction and the division are double, the result is
// rounded once on its store.  A row moves 20 / 12 / 8 bytes per entry (value + 4-byte index); a lane's gather of y is
// sizeof(S)*nc contiguous bytes.  The adjoint solve needs no kernel of its own: the host uploads the conjugate-transposed
// factors as a second resident set.
// ------------------------------------------------------------------------------------------------
typedef LuDevT<d2_t> CxLuDev;

template <bool LOWER, typename S>
__global__ __launch_bounds__(BLK) void cx_sptrsv_level(LuDevT<S> F, const int4* __restrict__ slots, int t0, int t1,
                                                       const S* __restrict__ b, S* y, int nrhs) {
  typedef typename lu_acc<S>::type A;
  const int t = t0 + (int)(((long long)blockIdx.x * BLK + threadIdx.x) >> 6);
  const int lane = threadIdx.x & 63;
  if (t >= t1) return;  // wave-uniform
  const int* __restrict__ col = LOWER ? F.Lcol : F.Ucol;
  const S* __restrict__ val = LOWER ? F.Lval : F.Uval;
  const int4 sl = slots[t];                       // (row, first and end of the off-diagonal entries, the diagonal entry)
  const int row = sl.x, s = sl.y, e = sl.z;
  const A dg = lu_wide(val[sl.w]);
  for (int c0 = 0; c0 < nrhs; c0 += 4) {
    const int nc = min(4, nrhs - c0);
    A acc[4] = {A{}, A{}, A{}, A{}};
    for (int k = s + lane; k < e; k += 64) {
      const A v = lu_wide(val[k]);
      const S* yy = y + (size_t)col[k] * nrhs + c0;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (u < nc) acc[u] += lu_mul(v, lu_wide(yy[u]));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      for (int o = 32; o > 0; o >>= 1) acc[u] += lu_shfl_xor(acc[u], o);
    if (lane < nc) {
      const A rhs = lu_wide(LOWER ? b[(size_t)F.p[row] * nrhs + c0 + lane] : y[(size_t)row * nrhs + c0 + lane]);
      const A a = lane == 0 ? acc[0] : lane == 1 ? acc[1] : lane == 2 ? acc[2] : acc[3];
      y[(size_t)row * nrhs + c0 + lane] = lu_round<S>(lu_div(rhs - a, dg));
    }
  }
}

// t = b[p] - L21*y1 for the rows n0.. of the trailing block of L
template <typename S>
__global__ __launch_bounds__(BLK) void cx_sptrsv_tail_rhs(LuDevT<S> F, int n0, const S* __restrict__ b,
                                                          const S* __restrict__ y, S* __restrict__ t, int nrhs) {
  typedef typename lu_acc<S>::type A;
  const int i = (int)(((long long)blockIdx.x * BLK + threadIdx.x) >> 6);
  const int lane = threadIdx.x & 63;
  const int row = n0 + i;
  if (row >= F.n) return;  // wave-uniform
  const int s = F.Lptr[row], e = F.Lptr[row + 1] - 1;
  for (int c0 = 0; c0 < nrhs; c0 += 4) {
    const int nc = min(4, nrhs - c0);
    A acc[4] = {A{}, A{}, A{}, A{}};
    for (int k = s + lane; k < e; k += 64) {
      const int c = F.Lcol[k];
      if (c >= n0) continue;                       // the trailing block itself is applied through its inverse
      const A v = lu_wide(F.Lval[k]);
      const S* yy = y + (size_t)c * nrhs + c0;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (u < nc) acc[u] += lu_mul(v, lu_wide(yy[u]));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      for (int o = 32; o > 0; o >>= 1) acc[u] += lu_shfl_xor(acc[u], o);
    if (lane < nc) {
      const A a = lane == 0 ? acc[0] : lane == 1 ? acc[1] : lane == 2 ? acc[2] : acc[3];
      t[(size_t)i * nrhs + c0 + lane] = lu_round<S>(lu_wide(b[(size_t)F.p[row] * nrhs + c0 + lane]) - a);
    }
  }
}

// x[q[r]] = y[r]
template <typename S>
__global__ __launch_bounds__(BLK) void cx_sptrsv_scatter(const int* __restrict__ q, const S* __restrict__ y,
                                                         S* __restrict__ x, int n, int nrhs) {
  const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
  if (i >= (long long)n * nrhs) return;
  const int r = (int)(i / nrhs), u = (int)(i - (long long)r * nrhs);
  x[(size_t)q[r] * nrhs + u] = y[i];
}

// Dense block (row-major, leading dimension ld = M rounded up to 64, zero outside the triangle, unit diagonal in the
// padding) of the rows/columns n0.. of a factor in CSR, widened to ComplexF64 whatever S is (a real value gets a zero
// imaginary part: the block is inverted by the one complex kernel below); D was zeroed by the host.
__device__ __forceinline__ d2_t tri_wide(d2_t a) { return a; }
__device__ __forceinline__ d2_t tri_wide(f2_t a) { return d2_t{(double)a.x, (double)a.y}; }
__device__ __forceinline__ d2_t tri_wide(float a) { return d2_t{(double)a, 0.0}; }
template <typename S>
__global__ __launch_bounds__(BLK) void cx_tri_gather_block(const int* __restrict__ ptr, const int* __restrict__ col,
                                                           const S* __restrict__ val, int n0, int M, int ld,
                                                           d2_t* __restrict__ D) {
  const int i = (int)(((long long)blockIdx.x * BLK + threadIdx.x) >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= ld) return;
  if (i >= M) {
    if (lane == 0) D[(size_t)i * ld + i] = d2_t{1.0, 0.0};
    return;
  }
  for (int k = ptr[n0 + i] + lane; k < ptr[n0 + i + 1]; k += 64) {
    const int c = col[k] - n0;
    if (c >= 0) D[(size_t)i * ld + c] = tri_wide(val[k]);
  }
}

// the ComplexF64 inverse of a single factor's trailing block rounded into its stored type (once, at setup)
__device__ __forceinline__ void tri_narrow(d2_t a, f2_t* o) { *o = f2_t{(float)a.x, (float)a.y}; }
__device__ __forceinline__ void tri_narrow(d2_t a, float* o) { *o = (float)a.x; }
template <typename S>
__global__ __launch_bounds__(BLK) void cx_tri_store(const d2_t* __restrict__ X, S* __restrict__ T, long long len) {
  const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
  if (i < len) tri_narrow(X[i], T + i);
}

// X = inv(D) for a dense complex triangular block (ld x ld, ld a multiple of 64): tri_inverse with 32 x 32 blocks
// (16-byte values: the four LDS tiles of the 64 x 64 form would not fit a workgroup).  One 256-thread workgroup per
// block of 32 columns of X walks the 32-row panels in substitution order; the contribution of the rows already known
// is a 32 x K x 32 product through LDS tiles (each thread a 2 x 2 register tile), the 32 x 32 diagonal block is then
// substituted in LDS by half a wavefront (a column per lane).  Setup-time kernel.
constexpr int CX_TRI_NB = 32;
template <bool LOWER>
__global__ __launch_bounds__(256) void cx_tri_inverse(const d2_t* __restrict__ D, d2_t* X, int ld) {
  constexpr int NB = CX_TRI_NB;
  __shared__ d2_t As[NB][17];
  __shared__ d2_t Bs[16][NB];
  __shared__ d2_t Ts[NB][NB + 1];
  __shared__ d2_t Ds[NB][NB + 1];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int C0 = blockIdx.x * NB, nP = ld / NB, cb = blockIdx.x;
  // rows outside the triangle of this column block
  for (int i = LOWER ? 0 : C0 + NB; i < (LOWER ? C0 : ld); i += 256 / NB) {
    const int r = i + tid / NB;
    if (r < (LOWER ? C0 : ld)) X[(size_t)r * ld + C0 + (tid & (NB - 1))] = d2_t{0.0, 0.0};
  }
  for (int pp = 0; pp < (LOWER ? nP - cb : cb + 1); ++pp) {
    const int p = LOWER ? cb + pp : cb - pp;
    const int I0 = p * NB;
    const int K0 = LOWER ? C0 : I0 + NB, K1 = LOWER ? I0 : C0 + NB;
    d2_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = d2_t{0.0, 0.0};
    for (int k0 = K0; k0 < K1; k0 += 16) {
      // D[I0 + r][k0 + kk]: 32 x 16; X[k0 + kk][C0 + c]: 16 x 32 - two elements per thread each
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int e = tid + 256 * u;
        As[e >> 4][e & 15] = D[(size_t)(I0 + (e >> 4)) * ld + k0 + (e & 15)];
        Bs[e / NB][e & (NB - 1)] = X[(size_t)(k0 + e / NB) * ld + C0 + (e & (NB - 1))];
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) {
        d2_t a[2], bb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = As[ty * 2 + i][kk];
#pragma unroll
        for (int j = 0; j < 2; ++j) bb[j] = Bs[kk][tx * 2 + j];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] += cmul(a[i], bb[j]);
      }
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int r = ty * 2 + i, c = tx * 2 + j;
        Ts[r][c] = d2_t{(I0 + r == C0 + c) ? 1.0 : 0.0, 0.0} - acc[i][j];
      }
    for (int e = tid; e < NB * NB; e += 256) Ds[e / NB][e & (NB - 1)] = D[(size_t)(I0 + e / NB) * ld + I0 + (e & (NB - 1))];
    __syncthreads();
    if (tid < NB) {                                 // within one wavefront, a column per lane: no barriers needed inside
      const int c = tid;
      if (LOWER) {
        for (int r = 0; r < NB; ++r) {
          d2_t v = Ts[r][c];
          for (int k = 0; k < r; ++k) v = v - cmul(Ds[r][k], Ts[k][c]);
          Ts[r][c] = cdiv(v, Ds[r][r]);
        }
      } else {
        for (int r = NB - 1; r >= 0; --r) {
          d2_t v = Ts[r][c];
          for (int k = r + 1; k < NB; ++k) v = v - cmul(Ds[r][k], Ts[k][c]);
          Ts[r][c] = cdiv(v, Ds[r][r]);
        }
      }
    }
    __syncthreads();
    for (int e = tid; e < NB * NB; e += 256) X[(size_t)(I0 + e / NB) * ld + C0 + (e & (NB - 1))] = Ts[e / NB][e & (NB - 1)];
    __threadfence();                                // the next panel of this workgroup reads these rows back
    __syncthreads();
  }
}

// x = T * b for a dense TRIANGULAR M x M block stored in S (row-major, leading dimension ld): one wavefront per (row, column),
// the sum in lu_acc<S>, rounded once
template <bool LOWER, typename S>
__global__ __launch_bounds__(BLK) void cx_tri_apply(const S* __restrict__ T, int ld, const S* __restrict__ b,
                                                    S* __restrict__ x, int M, int nrhs) {
  typedef typename lu_acc<S>::type A;
  const int wave = (int)(((long long)blockIdx.x * BLK + threadIdx.x) >> 6);
  const int lane = threadIdx.x & 63;
  if (wave >= M * nrhs) return;  // wave-uniform
  const int row = wave / nrhs, c = wave - row * nrhs;
  const S* __restrict__ a = T + (size_t)row * ld;
  const int j0 = LOWER ? 0 : (row & ~63), j1 = LOWER ? row + 1 : M;
  A acc = A{};
  for (int j = j0 + lane; j < j1; j += 64) acc += lu_mul(lu_wide(a[j]), lu_wide(b[(size_t)j * nrhs + c]));
  for (int o = 32; o > 0; o >>= 1) acc += lu_shfl_xor(acc, o);
  if (lane == 0) x[(size_t)row * nrhs + c] = lu_round<S>(acc);
}

// column-major n x nrhs (the host's layout) <-> row-major [n][nrhs] (the device's), entries of any value type
template <bool TO_ROWMAJOR, typename S>
__global__ __launch_bounds__(BLK) void cx_relayout(const S* __restrict__ src, S* __restrict__ dst, long long n, int nrhs) {
  const long long i = (long long)blockIdx.x * BLK + threadIdx.x;   // index into the row-major array
  if (i >= n * nrhs) return;
  const long long r = i / nrhs, c = i - r * nrhs;
  if (TO_ROWMAJOR) dst[i] = src[c * n + r];
  else dst[c * n + r] = src[i];
}

}  // namespace mgk
