// mg_dense_inv.inc - part of libmgvcycle.so's single translation unit (included by mgvcycle.hip; not compiled on its own).
// The dense inverse with partial pivoting on the device (kernels: mg_dense_inv.hpp): work set, the chain of launches, the flag.
// The host enqueues the whole inverse on one stream and synchronises once, when it reads the flag; the pivots never leave HBM.
namespace {

template <typename T>
struct DenseInv {
  static constexpr size_t D = sizeof(T) / sizeof(double);   // doubles per value
  int n = 0, ld = 0, nblk = 0;
  DevBuf<double> W, S0, S1, St, R, pv;   // work matrix ld x ld; the two strips ld x 64; strip transposed and pivot rows 64 x ld; partial keys
  DevBuf<int> pi, ipiv, src, flag;       // partial rows (two sets, as pv); pivots; column permutation; singular flag
  DenseInv() = default;
  DenseInv(const DenseInv&) = delete;
  ~DenseInv() { release(); }
  void release() {
    for (DevBuf<double>* d : {&W, &S0, &S1, &St, &R, &pv}) d->release();
    for (DevBuf<int>* d : {&pi, &ipiv, &src, &flag}) d->release();
  }
  T* w() { return reinterpret_cast<T*>(W.p); }
  // the work set of order n_, zeroed on `st` (the padding of W and of the strips stays zero throughout)
  int alloc(long long n_, hipStream_t st) {
    n = (int)n_;
    ld = (n + mgk::DI_NB - 1) / mgk::DI_NB * mgk::DI_NB;
    nblk = (n + mgk::DI_ROWS - 1) / mgk::DI_ROWS;
    const size_t strip = (size_t)ld * mgk::DI_NB * D;
    MG_TRY(W.alloc((size_t)ld * (size_t)ld * D));
    MG_TRY(S0.alloc(strip)); MG_TRY(S1.alloc(strip)); MG_TRY(St.alloc(strip)); MG_TRY(R.alloc(strip));
    MG_TRY(pv.alloc(2 * (size_t)nblk)); MG_TRY(pi.alloc(2 * (size_t)nblk));
    MG_TRY(ipiv.alloc((size_t)n)); MG_TRY(src.alloc((size_t)n)); MG_TRY(flag.alloc(1));
    for (DevBuf<double>* d : {&W, &S0, &S1, &St, &R}) HIP_TRY(hipMemsetAsync(d->p, 0, d->bytes(), st));
    HIP_TRY(hipMemsetAsync(ipiv.p, 0, ipiv.bytes(), st));
    HIP_TRY(hipMemsetAsync(flag.p, 0, flag.bytes(), st));
    return MG_OK;
  }
  // W holds the matrix: enqueue the inverse into `out` (row-major n x n).  n / 64 panels of 68 launches, no host synchronisation.
  int enqueue(T* out, hipStream_t st) {
    T* s[2] = {reinterpret_cast<T*>(S0.p), reinterpret_cast<T*>(S1.p)};
    T* st_t = reinterpret_cast<T*>(St.p);
    T* r = reinterpret_cast<T*>(R.p);
    const unsigned tiles = (unsigned)(ld / mgk::DI_NB);
    for (int k0 = 0; k0 < n; k0 += mgk::DI_NB) {
      const int nbw = std::min(mgk::DI_NB, n - k0);
      int cur = 0;
      hipLaunchKernelGGL(mgk::di_strip_load<T>, dim3((unsigned)nblk), dim3(256), 0, st, w(), ld, n, k0, s[0], pv.p, pi.p);
      for (int kk = 0; kk < nbw; ++kk, cur ^= 1)
        hipLaunchKernelGGL(mgk::di_step<T>, dim3((unsigned)nblk), dim3(256), 0, st, s[cur], s[cur ^ 1], n, k0, kk, pv.p + (size_t)cur * nblk,
                           pi.p + (size_t)cur * nblk, pv.p + (size_t)(cur ^ 1) * nblk, pi.p + (size_t)(cur ^ 1) * nblk, nblk, ipiv.p, flag.p);
      hipLaunchKernelGGL(mgk::di_swap_rows<T>, dim3((unsigned)((ld + mgk::BLK - 1) / mgk::BLK)), dim3(mgk::BLK), 0, st, w(), ld, k0, nbw, ipiv.p, r);
      hipLaunchKernelGGL(mgk::di_strip_store<T>, dim3((unsigned)(ld / mgk::DI_ROWS)), dim3(256), 0, st, s[cur], w(), st_t, ld, k0);
      if (tiles > 1) hipLaunchKernelGGL(mgk::di_update<T>, dim3(tiles, tiles), dim3(256), 0, st, w(), ld, st_t, r, k0);
      HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(mgk::di_perm, dim3(1), dim3(mgk::BLK), 0, st, ipiv.p, n, src.p);
    hipLaunchKernelGGL(mgk::di_gather<T>, dim3((unsigned)((n + mgk::BLK - 1) / mgk::BLK), (unsigned)n), dim3(mgk::BLK), 0, st, w(), ld, n, src.p, out);
    HIP_TRY(hipGetLastError());
    return MG_OK;
  }
  // behind the synchronisation: 0, or the 1-based column whose pivot was zero or not finite
  int singular_column(int* col) {
    HIP_TRY(hipMemcpy(col, flag.p, sizeof(int), hipMemcpyDeviceToHost));
    return MG_OK;
  }
};

// the largest order the device build serves on this handle
inline long long dense_inv_max(const Options& opt) { return std::max<long long>(0, std::min<long long>(opt.coarse_device_inverse_max, mgk::DI_MAX)); }

// the stand-alone inverse (mg_dense_inverse_FP64 / _CF64): host column-major in, host column-major out, one synchronisation
inline int dense_inverse_args(long long n, const double* A, const double* out, const char* who) {
  if (!A || !out) return fail(MG_ERR_INVALID, "%s: null argument", who);
  if (n < 1) return fail(MG_ERR_INVALID, "%s: n=%lld must be >= 1", who, n);
  if (n > mgk::DI_MAX) return fail(MG_ERR_UNSUPPORTED, "%s: order %lld exceeds %d", who, n, mgk::DI_MAX);
  return MG_OK;
}
// (the caller has checked the arguments and made the device current)
template <typename T>
int dense_inverse_host(long long n, const double* A, double* out, const char* who) {
  constexpr size_t D = DenseInv<T>::D;
  const size_t nn = (size_t)n * (size_t)n;
  DenseInv<T> K;
  DevBuf<double> a, x;
  struct Free { DevBuf<double>&a, &x; ~Free() { a.release(); x.release(); } } guard{a, x};
  MG_TRY(a.alloc(nn * D));
  MG_TRY(x.alloc(nn * D));
  HIP_TRY(hipMemcpy(a.p, A, nn * D * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipDeviceSynchronize());   // (the copy is ordered ahead of the kernels; not part of the inverse)
  MG_TRY(K.alloc(n, nullptr));
  const unsigned ge = (unsigned)((nn + mgk::BLK - 1) / mgk::BLK);
  hipLaunchKernelGGL(mgk::di_from_colmajor<T>, dim3(ge), dim3(mgk::BLK), 0, nullptr, reinterpret_cast<const T*>(a.p), (int)n, K.ld, K.w());
  MG_TRY(K.enqueue(reinterpret_cast<T*>(x.p), nullptr));
  hipLaunchKernelGGL(mgk::di_to_colmajor<T>, dim3(ge), dim3(mgk::BLK), 0, nullptr, reinterpret_cast<const T*>(x.p), (int)n, reinterpret_cast<T*>(a.p));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(nullptr));
  int col = 0;
  MG_TRY(K.singular_column(&col));
  if (col != 0) return fail(MG_ERR_INVALID, "%s: the matrix is singular to working precision (zero or non-finite pivot in column %d)", who, col);
  HIP_TRY(hipMemcpy(out, a.p, nn * D * sizeof(double), hipMemcpyDeviceToHost));
  return MG_OK;
}

// The coarsest operator's inverse from its resident CSR arrays, enqueued on `st` into `spare` (allocated here).  The caller
// synchronises, asks K.singular_column and exchanges `spare` with the installed inverse only when that is 0.
template <typename T, typename VT>
int coarse_inverse_enqueue(DenseInv<T>& K, DevBuf<double>& spare, long long n, const int* rowptr, const int* colidx, const VT* val, hipStream_t st) {
  MG_TRY(spare.alloc((size_t)n * (size_t)n * DenseInv<T>::D));
  MG_TRY(K.alloc(n, st));
  hipLaunchKernelGGL((mgk::di_scatter<T, VT>), dim3((unsigned)((n + mgk::BLK - 1) / mgk::BLK)), dim3(mgk::BLK), 0, st, rowptr, colidx, val, (int)n, K.ld, K.w());
  HIP_TRY(hipGetLastError());
  return K.enqueue(reinterpret_cast<T*>(spare.p), st);
}

// the installed inverse (row-major in HBM) to a host column-major array
template <size_t D>
int dense_inverse_readback(const DevBuf<double>& Ainv, long long n, double* out) {
  std::vector<double> rm((size_t)n * (size_t)n * D);
  HIP_TRY(hipMemcpy(rm.data(), Ainv.p, rm.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (long long i = 0; i < n; ++i)
    for (long long j = 0; j < n; ++j)
      for (size_t c = 0; c < D; ++c) out[D * ((size_t)j * n + i) + c] = rm[D * ((size_t)i * n + j) + c];
  return MG_OK;
}

}  // namespace
