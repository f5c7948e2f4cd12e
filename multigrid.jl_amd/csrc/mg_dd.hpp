// mg_dd.hpp - kernels of the multiplicative Schwarz sweep (mg_dd_*): the device form of solveDDSerial
// (src/DomainDecomposition/DDSerial.jl:108-139).  Per sub-domain i of the colour in turn:
//   r = (b - A x)[I_i]   (computeResidualAtIdx, DDSerial.jl:4-20),   t = A_i \ r   (solveSubDomain, l.183-187:
//   parallelJuliaSolver's x[q] = U \ (L \ r[p]), parLU.cpp:120-190),   x[I_i] += t   (l.129).
// Sub-domains of one colour that touch no common entry of x are one launch (dd_color_sweep: one 1024-thread workgroup
// per sub-domain, the three stages separated by workgroup barriers); otherwise the members run one after another
// (dd_gather_residual, the factor applier's solve, dd_scatter_add).  T = double, the interleaved complex d2_t, or their
// single twins float / f2_t.  A single handle STORES the operator, the factors, b, x, r and y in T and evaluates every
// residual row and every triangular row in lu_acc<T> (double / d2_t), as the single factor applier does (mg_kernels.hpp,
// sptrsv_sweep): operands widened on load - an f2_t moves as one 8-byte access -, the sum in the order of the double
// forms, one rounding on the store; x[I] += t is one add in T.  For double / d2_t widening and rounding are the identity.
#pragma once

namespace mgk {

// One sub-domain inside the packed arenas (all offsets in elements; row pointers, column indices, orders and
// permutations are local to the sub-domain, 0-based).
struct DdSub {
  int n;              // rows
  int vec0;           // index list, p, q, Lorder, Uorder and the work vectors: [vec0, vec0 + n)
  int ptr0;           // Lptr / Uptr: [ptr0, ptr0 + n + 1)
  int Lnz0, Unz0;     // first entry of Lcol / Lval and of Ucol / Uval
  int Llvl0, nLlvl;   // level pointers of L: [Llvl0, Llvl0 + nLlvl + 1)
  int Ulvl0, nUlvl;
};

template <typename T>
struct DdDevT {
  const int* rowptr; const int* col; const T* val;   // CSR of the applied operator A
  const int* idx;                                    // index lists I_i (0-based rows of A), packed
  const DdSub* sub;                                  // one descriptor per sub-domain
  const int* members;                                // sub-domains grouped by colour, linear order inside a colour
  const int* Lptr; const int* Lcol; const T* Lval; const int* Lorder; const int* Llvl;
  const int* Uptr; const int* Ucol; const T* Uval; const int* Uorder; const int* Ulvl;
  const int* p; const int* q;
  T* r; T* y;                                        // work vectors, packed like idx
};

// r[t] = b[I[t]] - sum_k val_k x[col_k] for t = first, first + step, ...: eight lanes share a row (rows of a grid
// operator hold 5-27 entries: a wavefront per row would leave most lanes idle), partial sums combined by shuffles.
template <typename T>
__device__ __forceinline__ void dd_residual_rows(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                 const T* __restrict__ val, const int* __restrict__ I, int n_i,
                                                 const T* __restrict__ b, const T* x, T* r, int first, int step) {
  const int part = threadIdx.x & 7;
  for (int t0 = first; t0 < n_i; t0 += step) {       // t0 is uniform over the eight lanes of a row
    const int row = I[t0];
    typename lu_acc<T>::type acc{};
    for (int k = rowptr[row] + part, e = rowptr[row + 1]; k < e; k += 8) acc += lu_mul(lu_wide(val[k]), lu_wide(x[col[k]]));
    for (int o = 4; o > 0; o >>= 1) acc += lu_shfl_xor(acc, o);
    if (part == 0) r[t0] = lu_round<T>(lu_wide(b[row]) - acc);
  }
}

// One launch per independent colour: workgroup g serves sub-domain members[m0 + g].
template <typename T>
__global__ __launch_bounds__(1024) void dd_color_sweep(DdDevT<T> D, int m0, const T* __restrict__ b, T* x) {
  __shared__ typename lu_acc<T>::type sred[16][4];   // what sptrsv_sweep combines split rows through
  const DdSub S = D.sub[D.members[m0 + blockIdx.x]];
  const int* I = D.idx + S.vec0;
  T* r = D.r + S.vec0;
  T* y = D.y + S.vec0;
  dd_residual_rows<T>(D.rowptr, D.col, D.val, I, S.n, b, x, r, (int)(threadIdx.x >> 3), (int)(blockDim.x >> 3));
  __syncthreads();
  sptrsv_sweep<true>(D.Lptr + S.ptr0, D.Lcol + S.Lnz0, D.Lval + S.Lnz0, D.Lorder + S.vec0, D.Llvl + S.Llvl0, S.nLlvl,
                     D.p + S.vec0, r, y, 1, 0, 1, sred);                                     // y = L \ r[p]
  sptrsv_sweep<false>(D.Uptr + S.ptr0, D.Ucol + S.Unz0, D.Uval + S.Unz0, D.Uorder + S.vec0, D.Ulvl + S.Ulvl0, S.nUlvl,
                      D.p + S.vec0, r, y, 1, 0, 1, sred);                                    // y = U \ y
  const int* q = D.q + S.vec0;
  for (int t = threadIdx.x; t < S.n; t += blockDim.x) {   // t[q] = y and x[I] += t in one pass
    const int g = I[q[t]];
    x[g] = x[g] + y[t];
  }
}

// The per-member sequence: r = (b - A x)[I] ...
template <typename T>
__global__ __launch_bounds__(BLK) void dd_gather_residual(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                          const T* __restrict__ val, const int* __restrict__ I, int n_i,
                                                          const T* __restrict__ b, const T* __restrict__ x,
                                                          T* __restrict__ r) {
  dd_residual_rows<T>(rowptr, col, val, I, n_i, b, x, r, (int)(((long long)blockIdx.x * BLK + threadIdx.x) >> 3),
                      (int)(((long long)gridDim.x * BLK) >> 3));
}

// ... and x[I] += t
template <typename T>
__global__ __launch_bounds__(BLK) void dd_scatter_add(const int* __restrict__ I, int n_i, const T* __restrict__ t,
                                                      T* __restrict__ x) {
  const int k = (int)((long long)blockIdx.x * BLK + threadIdx.x);
  if (k >= n_i) return;
  const int g = I[k];
  x[g] = x[g] + t[k];
}

}  // namespace mgk
