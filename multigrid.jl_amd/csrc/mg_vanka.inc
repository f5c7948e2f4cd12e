// mg_vanka.inc - part of libmgvcycle.so's single translation unit (included by mgvcycle.hip; not compiled on its own).
// The Vanka cell-block smoother of src/Multigrid/Vanka.jl on the device: the stand-alone handle (mg_vanka_*, extern "C"
// below) and the per-level form the cycle runs as relaxation type 2 (VankaCore, bound by mg_set_vanka_FP64, mg_cabi.inc, to a real
// level and by mg_set_vanka_CF64 / _CF32, mg_complex.inc, to a complex one).
// Kernels and the lane mapping: mg_vanka.hpp.
namespace {

constexpr int VANKA_FULL_RB = 1, VANKA_KACMARZ = 2, VANKA_ECON_RB = 3, VANKA_FULL_LEX = 4, VANKA_FULL_ADD = 5;   // Vanka.jl:13-17

// Geometry, the cells' blocks and the delta buffer: everything of the smoother but the operator's CSR arrays
struct VankaCore {
  mgk::VankaGeo G{};
  bool cx = false;
  bool single = false;     // cx only: the operator and the vectors hold float pairs (a level of a CF32 handle)
  DevBuf<float> D;         // LocalBlocks: bs*bs single-precision values per cell (complex: interleaved pairs)
  DevBuf<double> delta;    // cells x bs values of the operator's type (single: two of them per double slot)
  DevBuf<double> bdelta;   // the same for a block of bk columns: cells x bs x bk (vanka_block_ensure; empty until a block arrives)
  int bk = 0;
  long long launches = 0;  // kernels enqueued so far
  int colours_live = 0;    // colours that hold a cell (n[d] = 1 leaves the even parity of d empty)
  // the device build (vanka_build_launch / _finish): the blocks under construction, exchanged with D once a build has marked no cell;
  // {marked cells, the lowest of them}; and what the last successful build was asked for (has_w: D came from a build, not from the host)
  DevBuf<float> Dnew;
  DevBuf<int> flag;
  bool has_w = false;
  mgk::VankaBuild built{};
  void release() { D.release(); delta.release(); bdelta.release(); Dnew.release(); flag.release(); bk = 0; has_w = false; }
};

// (dim, n, includePressure) -> geometry; nrows must be sum(nf) [+ prod(n)] (getVankaBlockSize, Vanka.jl:211-222)
int vanka_geometry(long long dim, const long long* n, long long includePressure, long long nrows, mgk::VankaGeo* G) {
  if (dim != 2 && dim != 3) return fail(MG_ERR_INVALID, "dim=%lld: the face smoother serves 2-D and 3-D meshes", dim);
  if (!n) return fail(MG_ERR_INVALID, "n is null");
  if (includePressure != 0 && includePressure != 1) return fail(MG_ERR_INVALID, "includePressure must be 0 or 1");
  long long nn[3] = {n[0], n[1], dim == 3 ? n[2] : 1};
  for (int d = 0; d < 3; ++d)
    if (nn[d] < 1 || nn[d] >= (1LL << 30)) return fail(MG_ERR_INVALID, "n[%d]=%lld", d + 1, nn[d]);
  const long long cells = nn[0] * nn[1] * nn[2];
  const long long nf[3] = {(nn[0] + 1) * nn[1] * nn[2], nn[0] * (nn[1] + 1) * nn[2], dim == 3 ? nn[0] * nn[1] * (nn[2] + 1) : 0};
  const long long N = nf[0] + nf[1] + nf[2] + (includePressure ? cells : 0);
  if (N >= (1LL << 31) - 1 || cells * 8 >= (1LL << 40)) return fail(MG_ERR_UNSUPPORTED, "the mesh exceeds int32 device indices");
  if (nrows != N) return fail(MG_ERR_INVALID, "the operator has %lld rows, but a mesh of %lldx%lldx%lld cells has %lld unknowns (includePressure=%lld)", nrows, nn[0], nn[1], nn[2], N, includePressure);
  G->dim = (int)dim;
  G->ip = (int)includePressure;
  G->bs = 2 * (int)dim + (int)includePressure;
  for (int d = 0; d < 3; ++d) { G->n[d] = (int)nn[d]; G->nf[d] = (int)nf[d]; }
  G->cells = (int)cells;
  G->N = (int)N;
  return MG_OK;
}

int vanka_type_served(long long type) {
  if (type == VANKA_FULL_RB || type == VANKA_ECON_RB || type == VANKA_FULL_ADD) return MG_OK;
  if (type == VANKA_FULL_LEX) return fail(MG_ERR_UNSUPPORTED, "FULL_VANKA_LEX is a sequential sweep over the cells: not served on the device");
  if (type == VANKA_KACMARZ) return fail(MG_ERR_UNSUPPORTED, "KACMARZ_VANKA belongs to the hybrid cell-wise path: not served");
  return fail(MG_ERR_UNSUPPORTED, "unknown Vanka type %lld", type);
}

// floats of the cells' blocks
inline size_t vanka_block_floats(const VankaCore* V) {
  return (V->cx ? 2 : 1) * (size_t)V->G.bs * (size_t)V->G.bs * (size_t)V->G.cells;
}

// geometry and buffers of a core; the blocks arrive from the host (vanka_core_init) or from a build (vanka_build_launch)
int vanka_core_alloc(VankaCore* V, bool cx, const mgk::VankaGeo& G, bool single = false) {
  const size_t vw = cx ? 2 : 1;
  V->G = G;
  V->cx = cx;
  V->single = cx && single;
  V->colours_live = 1;
  for (int d = 0; d < G.dim; ++d) V->colours_live *= G.n[d] >= 2 ? 2 : 1;
  MG_TRY(V->D.alloc(vanka_block_floats(V)));
  MG_TRY(V->delta.alloc((V->single ? 1 : vw) * (size_t)G.bs * (size_t)G.cells));
  return MG_OK;
}

// D_blocks: (bs*bs) x cells column-major, Float32 (cx: ComplexF32) - the caller's LocalBlocks as they are
int vanka_core_init(VankaCore* V, bool cx, const mgk::VankaGeo& G, const void* D_blocks, bool single = false) {
  if (!D_blocks) return fail(MG_ERR_INVALID, "D_blocks is null");
  MG_TRY(vanka_core_alloc(V, cx, G, single));
  HIP_TRY(hipMemcpy(V->D.p, D_blocks, vanka_block_floats(V) * sizeof(float), hipMemcpyHostToDevice));
  return MG_OK;
}

// ---- the blocks built on the device (kernel: vanka_build_blocks, mg_vanka.hpp) ------------------------------------------------------
// (VankaType, w[nw]) of a build: types as vanka_type_served; nw = 1 (a scalar w) or 2 (the pair (w0, w1)); ECON_VANKA_RB divides the
// diagonal by its one w (Vanka.jl:361), so a pair is refused, as setupVankaFacesPreconditioner refuses it
int vanka_build_args(long long type, const double* w, long long nw, mgk::VankaBuild* P) {
  MG_TRY(vanka_type_served(type));
  if (!w) return fail(MG_ERR_INVALID, "w is null");
  if (nw != 1 && nw != 2) return fail(MG_ERR_INVALID, "nw=%lld: w is one number or a pair", nw);
  if (type == VANKA_ECON_RB && nw == 2) return fail(MG_ERR_INVALID, "ECON_VANKA_RB takes a scalar w (nw = 1)");
  P->type = (int)type;
  P->scalar = nw == 1 ? 1 : 0;
  P->w0 = w[0];
  P->w1 = nw == 2 ? w[1] : w[0];
  return MG_OK;
}

// Enqueue one build of the core's blocks from the CSR of its operator (val: double, or interleaved pairs of doubles, or of floats where
// V->single) into V->Dnew; V->D and whatever relaxes with it are not touched.  vanka_build_finish, after the caller has waited for the
// stream, makes them the core's blocks.
int vanka_build_launch(VankaCore* V, const int* rowptr, const int* col, const void* val, const mgk::VankaBuild& P, hipStream_t stream) {
  const mgk::VankaGeo& G = V->G;
  const size_t nD = vanka_block_floats(V);
  if (V->Dnew.n != nD) MG_TRY(V->Dnew.alloc(nD));
  if (V->flag.n != 2) MG_TRY(V->flag.alloc(2));
  HIP_TRY(hipMemsetAsync(V->flag.p, 0, 2 * sizeof(int), stream));
  const dim3 grid((unsigned)(((long long)G.cells * 8 + mgk::BLK - 1) / mgk::BLK)), block(mgk::BLK);
  if (!V->cx)
    hipLaunchKernelGGL(mgk::vanka_build_blocks<double>, grid, block, 0, stream, G, P, rowptr, col, static_cast<const double*>(val), V->Dnew.p,
                       V->flag.p);
  else if (V->single)
    hipLaunchKernelGGL(mgk::vanka_build_blocks<mgk::f2_t>, grid, block, 0, stream, G, P, rowptr, col, static_cast<const mgk::f2_t*>(val),
                       reinterpret_cast<float2*>(V->Dnew.p), V->flag.p);
  else
    hipLaunchKernelGGL(mgk::vanka_build_blocks<mgk::d2_t>, grid, block, 0, stream, G, P, rowptr, col, static_cast<const mgk::d2_t*>(val),
                       reinterpret_cast<float2*>(V->Dnew.p), V->flag.p);
  ++V->launches;
  HIP_TRY(hipGetLastError());
  return MG_OK;
}

// The stream of the build has been waited for.  No cell marked: the new blocks become the core's and (type, w) are remembered.
// Otherwise the core keeps its blocks; *bad_cells and *first_cell (0-based) say what was found.
int vanka_build_finish(VankaCore* V, const mgk::VankaBuild& P, int* bad_cells, int* first_cell) {
  int flag[2] = {0, 0};
  HIP_TRY(hipMemcpy(flag, V->flag.p, sizeof(flag), hipMemcpyDeviceToHost));
  *bad_cells = flag[0];
  *first_cell = INT_MAX - flag[1];   // (the kernel keeps the maximum of INT_MAX - cell: a zero-filled flag needs no other start value)
  if (flag[0] != 0) return MG_OK;
  std::swap(V->D.p, V->Dnew.p);   // (both hold vanka_block_floats values)
  V->has_w = true;
  V->built = P;
  return MG_OK;
}

int vanka_singular(int bad_cells, int first_cell, const char* where) {
  return fail(MG_ERR_INVALID, "%s: the block of cell %d is singular (a zero or non-finite pivot; %d such cell%s): the previous blocks are kept",
              where, first_cell + 1, bad_cells, bad_cells == 1 ? "" : "s");
}

// numit relaxations of x (in place) on `stream`, no synchronisation.  The caller has checked the type (vanka_type_served).
// ZERO: x holds zeros on entry (the caller zero-filled it), so the first snapshot's residual is b[I] and its pass walks no matrix row
// (vanka_delta<T, true>): the first colour of the first iteration, or the one pass of FULL_VANKA_ADD.
template <typename T, bool ZERO = false>
int vanka_sweeps(VankaCore* V, const int* rowptr, const int* col, const T* val, const T* b, T* x, long long numit, int type,
                 hipStream_t stream) {
  typedef typename mgk::VankaBlk<T>::type B;
  const mgk::VankaGeo& G = V->G;
  const B* D = reinterpret_cast<const B*>(V->D.p);
  T* delta = reinterpret_cast<T*>(V->delta.p);
  if (numit <= 0) return MG_OK;   // numit = 0 does nothing (Vanka.jl:397,408), unlike relax
  auto blocks = [](long long groups) { return dim3((unsigned)((groups * 8 + mgk::BLK - 1) / mgk::BLK)); };
  if (type == VANKA_FULL_ADD) {
    // y = copy(x) once per call (Vanka.jl:396): every iteration adds the same corrections
    hipLaunchKernelGGL((mgk::vanka_delta<T, ZERO>), blocks(G.cells), dim3(mgk::BLK), 0, stream, G, rowptr, col, val, D, b, x, delta, G.cells,
                       G.n[0], G.n[1], 0, 0, 0, 1);
    ++V->launches;
    for (long long it = 0; it < numit; ++it) {
      hipLaunchKernelGGL(mgk::vanka_apply_add<T>, dim3((unsigned)(((long long)G.N + mgk::BLK - 1) / mgk::BLK)), dim3(mgk::BLK), 0, stream, G,
                         delta, x);
      ++V->launches;
    }
    HIP_TRY(hipGetLastError());
    return MG_OK;
  }
  const int ncol = 1 << G.dim;
  bool from_zero = ZERO;   // until the first colour has been applied
  for (long long it = 0; it < numit; ++it)
    for (int c = 0; c < ncol; ++c) {
      // cellColor (Vanka.jl:105-127): the first dimension's parity is the most significant bit; odd 1-based = even 0-based first
      int p[3] = {0, 0, 0}, m[3] = {1, 1, 1};
      for (int d = 0; d < G.dim; ++d) {
        p[d] = (c >> (G.dim - 1 - d)) & 1;
        m[d] = (G.n[d] + 1 - p[d]) / 2;
      }
      const long long count = (long long)m[0] * m[1] * m[2];
      if (count == 0) continue;
      if (ZERO && from_zero)
        hipLaunchKernelGGL((mgk::vanka_delta<T, ZERO>), blocks(count), dim3(mgk::BLK), 0, stream, G, rowptr, col, val, D, b, x, delta, (int)count,
                           m[0], m[1], p[0], p[1], p[2], 0);
      else
        hipLaunchKernelGGL((mgk::vanka_delta<T, false>), blocks(count), dim3(mgk::BLK), 0, stream, G, rowptr, col, val, D, b, x, delta, (int)count,
                           m[0], m[1], p[0], p[1], p[2], 0);
      from_zero = false;
      hipLaunchKernelGGL(mgk::vanka_apply_colour<T>, blocks(count), dim3(mgk::BLK), 0, stream, G, delta, x, (int)count, m[0], m[1], p[0],
                         p[1], p[2]);
      V->launches += 2;
    }
  HIP_TRY(hipGetLastError());
  return MG_OK;
}

int vanka_run(VankaCore* V, const int* rowptr, const int* col, const double* val, const double* b, double* x, long long numit, int type,
              hipStream_t stream) {
  if (V->cx)
    return vanka_sweeps<mgk::d2_t>(V, rowptr, col, reinterpret_cast<const mgk::d2_t*>(val), reinterpret_cast<const mgk::d2_t*>(b),
                                   reinterpret_cast<mgk::d2_t*>(x), numit, type, stream);
  return vanka_sweeps<double>(V, rowptr, col, val, b, x, numit, type, stream);
}

// The delta buffer of the block passes for k columns: grown when a larger k arrives (the caller has waited for the stream that may
// still read the old one), kept with the core.  A complex level's grows with the handle's block work set (cx_block_ensure).
int vanka_block_ensure(VankaCore* V, int k) {
  if (k <= V->bk) return MG_OK;
  V->bk = 0;
  MG_TRY(V->bdelta.alloc((V->single || !V->cx ? 1 : 2) * (size_t)V->G.bs * (size_t)V->G.cells * (size_t)k));
  V->bk = k;
  return MG_OK;
}

// vanka_sweeps on a row-major block [N][k] (kernels: the _blk forms of mg_vanka.hpp): the same launches in the same order, each serving
// all k columns.  ZERO is a property of the whole block.
template <typename T, bool ZERO = false>
int vanka_sweeps_blk(VankaCore* V, const int* rowptr, const int* col, const T* val, const T* b, T* x, int k, long long numit, int type,
                     hipStream_t stream) {
  typedef typename mgk::VankaBlk<T>::type B;
  const mgk::VankaGeo& G = V->G;
  if (k < 1 || k > mgk::BLK_KMAX) return fail(MG_ERR_INVALID, "internal: a Vanka block of %d columns", k);
  if (V->bk < k) return fail(MG_ERR_STATE, "internal: the Vanka delta buffer holds %d columns, the block %d", V->bk, k);
  const B* D = reinterpret_cast<const B*>(V->D.p);
  T* delta = reinterpret_cast<T*>(V->bdelta.p);
  if (numit <= 0) return MG_OK;
  // lanes of the largest launch, in 64 bits: all cells (or all unknowns) times k
  const long long most = std::max((long long)G.cells * 8, (long long)G.N) * k;
  if ((most + mgk::BLK - 1) / mgk::BLK >= (1LL << 31)) return fail(MG_ERR_UNSUPPORTED, "the mesh times %d columns exceeds the launch grid", k);
  auto blocks = [k](long long groups) { return dim3((unsigned)((groups * 8 * k + mgk::BLK - 1) / mgk::BLK)); };
  if (type == VANKA_FULL_ADD) {
    hipLaunchKernelGGL((mgk::vanka_delta_blk<T, ZERO>), blocks(G.cells), dim3(mgk::BLK), 0, stream, G, rowptr, col, val, D, b, x, delta, k,
                       G.cells, G.n[0], G.n[1], 0, 0, 0, 1);
    ++V->launches;
    for (long long it = 0; it < numit; ++it) {
      hipLaunchKernelGGL(mgk::vanka_apply_add_blk<T>, dim3((unsigned)(((long long)G.N * k + mgk::BLK - 1) / mgk::BLK)), dim3(mgk::BLK), 0, stream,
                         G, delta, x, k);
      ++V->launches;
    }
    HIP_TRY(hipGetLastError());
    return MG_OK;
  }
  const int ncol = 1 << G.dim;
  bool from_zero = ZERO;   // until the first colour has been applied
  for (long long it = 0; it < numit; ++it)
    for (int c = 0; c < ncol; ++c) {
      int p[3] = {0, 0, 0}, m[3] = {1, 1, 1};   // cellColor, as vanka_sweeps
      for (int d = 0; d < G.dim; ++d) {
        p[d] = (c >> (G.dim - 1 - d)) & 1;
        m[d] = (G.n[d] + 1 - p[d]) / 2;
      }
      const long long count = (long long)m[0] * m[1] * m[2];
      if (count == 0) continue;
      if (ZERO && from_zero)
        hipLaunchKernelGGL((mgk::vanka_delta_blk<T, ZERO>), blocks(count), dim3(mgk::BLK), 0, stream, G, rowptr, col, val, D, b, x, delta, k,
                           (int)count, m[0], m[1], p[0], p[1], p[2], 0);
      else
        hipLaunchKernelGGL((mgk::vanka_delta_blk<T, false>), blocks(count), dim3(mgk::BLK), 0, stream, G, rowptr, col, val, D, b, x, delta, k,
                           (int)count, m[0], m[1], p[0], p[1], p[2], 0);
      from_zero = false;
      hipLaunchKernelGGL(mgk::vanka_apply_colour_blk<T>, blocks(count), dim3(mgk::BLK), 0, stream, G, delta, x, k, (int)count, m[0], m[1],
                         p[0], p[1], p[2]);
      V->launches += 2;
    }
  HIP_TRY(hipGetLastError());
  return MG_OK;
}

int vanka_run_blk(VankaCore* V, const int* rowptr, const int* col, const double* val, const double* b, double* x, int k, long long numit,
                  int type, hipStream_t stream) {
  if (V->cx)
    return vanka_sweeps_blk<mgk::d2_t>(V, rowptr, col, reinterpret_cast<const mgk::d2_t*>(val), reinterpret_cast<const mgk::d2_t*>(b),
                                       reinterpret_cast<mgk::d2_t*>(x), k, numit, type, stream);
  return vanka_sweeps_blk<double>(V, rowptr, col, val, b, x, k, numit, type, stream);
}

// The same on a level of a complex hierarchy: C = mgk::d2_t (a CF64 handle) or mgk::f2_t (a CF32 handle, V->single).  xzero: the caller
// has zero-filled x (a level entered from zero): the from-zero pass opens the call.
template <typename C>
int vanka_run_cx(VankaCore* V, const int* rowptr, const int* col, const C* val, const C* b, C* x, long long numit, int type, bool xzero,
                 hipStream_t stream) {
  if (!V->cx || V->single != (sizeof(C) == sizeof(mgk::f2_t))) return fail(MG_ERR_INVALID, "internal: Vanka blocks and vectors differ in type");
  if (xzero) return vanka_sweeps<C, true>(V, rowptr, col, val, b, x, numit, type, stream);
  return vanka_sweeps<C, false>(V, rowptr, col, val, b, x, numit, type, stream);
}

// vanka_run_cx on a row-major block of k columns (the block cycle of a complex handle, option vanka_blocks)
template <typename C>
int vanka_run_cx_blk(VankaCore* V, const int* rowptr, const int* col, const C* val, const C* b, C* x, int k, long long numit, int type,
                     bool xzero, hipStream_t stream) {
  if (!V->cx || V->single != (sizeof(C) == sizeof(mgk::f2_t))) return fail(MG_ERR_INVALID, "internal: Vanka blocks and vectors differ in type");
  if (xzero) return vanka_sweeps_blk<C, true>(V, rowptr, col, val, b, x, k, numit, type, stream);
  return vanka_sweeps_blk<C, false>(V, rowptr, col, val, b, x, k, numit, type, stream);
}

}  // namespace

struct mg_vanka {
  int device = 0;
  long long n = 0, nnz = 0;
  VankaCore core;
  DevBuf<int> rowptr, col;
  DevBuf<double> val, stage_x, stage_b;
  DevBuf<double> bstage_x, bstage_b;   // the block entries' row-major blocks (host forms)
  hipStream_t stream = nullptr;
};

namespace {

int vanka_build_handle(mg_vanka* v, const mgk::VankaBuild& P, const char* name);

// D_blocks: the caller's blocks, or null with `build`: the blocks are built on the device from the operator just uploaded
int vanka_create(bool cx, long long device_id, long long dim, const long long* n, long long includePressure, long long nrows,
                 const long long* rowptr, const long long* colA, const double* valA, const void* D_blocks, mg_vanka** out,
                 const mgk::VankaBuild* build = nullptr) {
  const size_t vw = cx ? 2 : 1;
  if (!out) return fail(MG_ERR_INVALID, "out is null");
  *out = nullptr;
  if (nrows < 1 || !rowptr || !colA || !valA || (!D_blocks && !build)) return fail(MG_ERR_INVALID, "null or empty argument");
  mgk::VankaGeo G;
  MG_TRY(vanka_geometry(dim, n, includePressure, nrows, &G));
  if (rowptr[0] != 1) return fail(MG_ERR_INVALID, "rowptr[1] must be 1 (1-based Julia arrays expected)");
  const long long nnz = rowptr[nrows] - 1;
  if (nnz < 0 || nnz >= (1LL << 31) - 1) return fail(MG_ERR_UNSUPPORTED, "nnz does not fit int32");
  std::vector<int> rp((size_t)nrows + 1), ci((size_t)std::max<long long>(nnz, 1));
  for (long long i = 0; i <= nrows; ++i) {
    const long long v = rowptr[i] - 1;
    if (v < 0 || v > nnz || (i > 0 && v < rp[(size_t)i - 1])) return fail(MG_ERR_INVALID, "rowptr is not a monotone 1-based pointer array");
    rp[(size_t)i] = (int)v;
  }
  for (long long k = 0; k < nnz; ++k) {
    const long long c = colA[k] - 1;
    if (c < 0 || c >= nrows) return fail(MG_ERR_INVALID, "column index out of range");
    ci[(size_t)k] = (int)c;
  }
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (ndev <= 0) return fail(MG_ERR_HIP, "no HIP device visible: the Vanka smoother has no CPU fallback");
  if (device_id < 0 || device_id >= ndev) return fail(MG_ERR_INVALID, "device_id=%lld but %d devices visible", device_id, ndev);
  HIP_TRY(hipSetDevice((int)device_id));
  mg_vanka* v = new mg_vanka();
  v->device = (int)device_id;
  v->n = nrows;
  v->nnz = nnz;
  auto up = [&]() -> int {
    MG_TRY(v->rowptr.alloc(rp.size()));
    MG_TRY(v->col.alloc(ci.size()));
    MG_TRY(v->val.alloc(vw * (size_t)std::max<long long>(nnz, 1)));
    HIP_TRY(hipMemcpy(v->rowptr.p, rp.data(), rp.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(v->col.p, ci.data(), (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(v->val.p, valA, vw * (size_t)nnz * sizeof(double), hipMemcpyHostToDevice));
    if (build) MG_TRY(vanka_core_alloc(&v->core, cx, G));
    else MG_TRY(vanka_core_init(&v->core, cx, G, D_blocks));
    HIP_TRY(hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking));
    return MG_OK;
  };
  int rc = up();
  (void)hipDeviceSynchronize();   // the blocking copies above ran on the NULL stream; the kernels run on the handle's own
  if (rc == MG_OK && build) rc = vanka_build_handle(v, *build, "mg_vanka_create_built");
  if (rc != MG_OK) {
    mg_vanka_destroy(v);
    return rc;
  }
  *out = v;
  return MG_OK;
}

// The arguments of an apply and the handle's value type (cx: the entry point's)
int vanka_args(bool cx, mg_vanka* v, const double* x, const double* b, long long numit, long long type, const char* name) {
  if (!v) return fail(MG_ERR_INVALID, "null handle");
  if (v->core.cx != cx)
    return fail(MG_ERR_STATE, "%s on a handle of %s values (%s)", name, v->core.cx ? "ComplexF64" : "Float64",
                v->core.cx ? "mg_vanka_apply*_CFP64" : "mg_vanka_apply*_FP64");
  if (!x || !b || x == b || numit < 0) return fail(MG_ERR_INVALID, "bad argument (x and b must be two vectors, numit >= 0)");
  MG_TRY(vanka_type_served(type));
  (void)hipSetDevice(v->device);
  return MG_OK;
}

int vanka_apply_dev(bool cx, mg_vanka* v, double* x_dev, const double* b_dev, long long numit, long long type, const char* name) {
  MG_TRY(vanka_args(cx, v, x_dev, b_dev, numit, type, name));
  MG_TRY(vanka_run(&v->core, v->rowptr.p, v->col.p, v->val.p, b_dev, x_dev, numit, (int)type, v->stream));
  HIP_TRY(spin_sync(v->stream));
  return MG_OK;
}

int vanka_apply_host(bool cx, mg_vanka* v, double* x, const double* b, long long numit, long long type, const char* name) {
  MG_TRY(vanka_args(cx, v, x, b, numit, type, name));
  if (numit == 0) return MG_OK;
  const size_t len = (cx ? 2 : 1) * (size_t)v->n;   // doubles
  if (v->stage_x.n != len) {
    MG_TRY(v->stage_x.alloc(len));
    MG_TRY(v->stage_b.alloc(len));
  }
  HIP_TRY(hipMemcpyAsync(v->stage_x.p, x, len * sizeof(double), hipMemcpyHostToDevice, v->stream));
  HIP_TRY(hipMemcpyAsync(v->stage_b.p, b, len * sizeof(double), hipMemcpyHostToDevice, v->stream));
  MG_TRY(vanka_run(&v->core, v->rowptr.p, v->col.p, v->val.p, v->stage_b.p, v->stage_x.p, numit, (int)type, v->stream));
  HIP_TRY(hipMemcpyAsync(x, v->stage_x.p, len * sizeof(double), hipMemcpyDeviceToHost, v->stream));
  HIP_TRY(spin_sync(v->stream));
  return MG_OK;
}

// ---- blocks of right-hand sides on the stand-alone handle (mg_vanka_apply_block_*) -------------------------------------------------
int vanka_block_args(bool cx, mg_vanka* v, const double* x, const double* b, long long nrhs, long long numit, long long type, const char* name) {
  if (!v) return fail(MG_ERR_INVALID, "null handle");
  if (nrhs < 1) return fail(MG_ERR_INVALID, "nrhs=%lld: a block holds at least one right-hand side", nrhs);
  if (nrhs > mgk::BLK_KMAX) return fail(MG_ERR_UNSUPPORTED, "Vanka blocks hold at most %d right-hand sides (nrhs=%lld)", mgk::BLK_KMAX, nrhs);
  MG_TRY(vanka_args(cx, v, x, b, numit, type, name));
  if (v->core.bk < (int)nrhs) {
    HIP_TRY(spin_sync(v->stream));   // (an earlier block call may still read the buffer replaced below)
    MG_TRY(vanka_block_ensure(&v->core, (int)nrhs));
  }
  return MG_OK;
}

int vanka_apply_block_dev(bool cx, mg_vanka* v, double* x_dev, const double* b_dev, long long nrhs, long long numit, long long type,
                          const char* name) {
  MG_TRY(vanka_block_args(cx, v, x_dev, b_dev, nrhs, numit, type, name));
  MG_TRY(vanka_run_blk(&v->core, v->rowptr.p, v->col.p, v->val.p, b_dev, x_dev, (int)nrhs, numit, (int)type, v->stream));
  HIP_TRY(spin_sync(v->stream));
  return MG_OK;
}

// x, b: column-major N x nrhs on the host; relaid to row-major on the host (a stand-alone entry: nothing of it is on a hot path)
int vanka_apply_block_host(bool cx, mg_vanka* v, double* x, const double* b, long long nrhs, long long numit, long long type,
                           const char* name) {
  MG_TRY(vanka_block_args(cx, v, x, b, nrhs, numit, type, name));
  if (numit == 0) return MG_OK;
  const size_t vw = cx ? 2 : 1, n = (size_t)v->n, k = (size_t)nrhs, len = vw * n * k;   // doubles
  if (v->bstage_x.n < len) {
    HIP_TRY(spin_sync(v->stream));
    MG_TRY(v->bstage_x.alloc(len));
    MG_TRY(v->bstage_b.alloc(len));
  }
  std::vector<double> rx(len), rb(len);
  for (size_t c = 0; c < k; ++c)
    for (size_t i = 0; i < n; ++i)
      for (size_t w = 0; w < vw; ++w) {
        rx[(i * k + c) * vw + w] = x[(c * n + i) * vw + w];
        rb[(i * k + c) * vw + w] = b[(c * n + i) * vw + w];
      }
  HIP_TRY(hipMemcpyAsync(v->bstage_x.p, rx.data(), len * sizeof(double), hipMemcpyHostToDevice, v->stream));
  HIP_TRY(hipMemcpyAsync(v->bstage_b.p, rb.data(), len * sizeof(double), hipMemcpyHostToDevice, v->stream));
  MG_TRY(vanka_run_blk(&v->core, v->rowptr.p, v->col.p, v->val.p, v->bstage_b.p, v->bstage_x.p, (int)nrhs, numit, (int)type, v->stream));
  HIP_TRY(hipMemcpyAsync(rx.data(), v->bstage_x.p, len * sizeof(double), hipMemcpyDeviceToHost, v->stream));
  HIP_TRY(spin_sync(v->stream));
  for (size_t c = 0; c < k; ++c)
    for (size_t i = 0; i < n; ++i)
      for (size_t w = 0; w < vw; ++w) x[(c * n + i) * vw + w] = rx[(i * k + c) * vw + w];
  return MG_OK;
}

// ---- the blocks of the stand-alone handle built from its resident operator ----------------------------------------------------------
int vanka_build_handle(mg_vanka* v, const mgk::VankaBuild& P, const char* name) {
  (void)hipSetDevice(v->device);
  HIP_TRY(spin_sync(v->stream));   // (an earlier build's buffer may still be read)
  MG_TRY(vanka_build_launch(&v->core, v->rowptr.p, v->col.p, v->val.p, P, v->stream));
  HIP_TRY(spin_sync(v->stream));
  int bad = 0, first = 0;
  MG_TRY(vanka_build_finish(&v->core, P, &bad, &first));
  return bad ? vanka_singular(bad, first, name) : MG_OK;
}

int vanka_handle_type(bool cx, mg_vanka* v, const char* name) {
  if (!v) return fail(MG_ERR_INVALID, "null handle");
  if (v->core.cx != cx)
    return fail(MG_ERR_STATE, "%s on a handle of %s values (%s)", name, v->core.cx ? "ComplexF64" : "Float64", v->core.cx ? "the _CFP64 form" : "the _FP64 form");
  return MG_OK;
}

int vanka_build_entry(bool cx, mg_vanka* v, long long type, const double* w, long long nw, const char* name) {
  MG_TRY(vanka_handle_type(cx, v, name));
  mgk::VankaBuild P;
  MG_TRY(vanka_build_args(type, w, nw, &P));
  return vanka_build_handle(v, P, name);
}

int vanka_replace_values(bool cx, mg_vanka* v, const double* nzval, long long nnz, const char* name) {
  MG_TRY(vanka_handle_type(cx, v, name));
  if (!nzval) return fail(MG_ERR_INVALID, "nzval is null");
  if (nnz != v->nnz) return fail(MG_ERR_INVALID, "nnz=%lld differs from the stored pattern (%lld)", nnz, v->nnz);
  (void)hipSetDevice(v->device);
  HIP_TRY(spin_sync(v->stream));
  if (nnz > 0) HIP_TRY(hipMemcpy(v->val.p, nzval, (cx ? 2 : 1) * (size_t)nnz * sizeof(double), hipMemcpyHostToDevice));
  return MG_OK;
}

int vanka_create_built(bool cx, long long device_id, long long dim, const long long* n, long long includePressure, long long nrows,
                       const long long* rowptr, const long long* colA, const double* valA, long long type, const double* w, long long nw,
                       mg_vanka** out) {
  if (out) *out = nullptr;
  mgk::VankaBuild P;
  MG_TRY(vanka_build_args(type, w, nw, &P));
  return vanka_create(cx, device_id, dim, n, includePressure, nrows, rowptr, colA, valA, nullptr, out, &P);
}

}  // namespace

extern "C" {

// rowptr / colA / valA: CSR of the applied operator A (1-based Int64; valA the values of A's rows - the reference's
// conj(AT.nzval), computeResidualAtIdx, Vanka.jl:192-198).  n[dim]: cells of the RegularMesh.  D_blocks: LocalBlocks of
// setupVankaFacesPreconditioner (Vanka.jl:294-370), (bs*bs) x prod(n) column-major Float32 (CFP64: ComplexF32).
int mg_vanka_create_FP64_INT64(long long device_id, long long dim, const long long* n, long long includePressure, long long nrows,
                               const long long* rowptr, const long long* colA, const double* valA, const float* D_blocks, mg_vanka** out) {
  return vanka_create(false, device_id, dim, n, includePressure, nrows, rowptr, colA, valA, D_blocks, out);
}
int mg_vanka_create_CFP64_INT64(long long device_id, long long dim, const long long* n, long long includePressure, long long nrows,
                                const long long* rowptr, const long long* colA, const double* valA, const float* D_blocks, mg_vanka** out) {
  return vanka_create(true, device_id, dim, n, includePressure, nrows, rowptr, colA, valA, D_blocks, out);
}

// The blocks built on the device (kernel: vanka_build_blocks, mg_vanka.hpp) instead of handed over: see include/mgvcycle.h.
// mg_vanka_create_built_*: the create call with (VankaType, w[nw]) in the place of D_blocks.
int mg_vanka_create_built_FP64_INT64(long long device_id, long long dim, const long long* n, long long includePressure, long long nrows,
                                     const long long* rowptr, const long long* colA, const double* valA, long long VankaType, const double* w,
                                     long long nw, mg_vanka** out) {
  return vanka_create_built(false, device_id, dim, n, includePressure, nrows, rowptr, colA, valA, VankaType, w, nw, out);
}
int mg_vanka_create_built_CFP64_INT64(long long device_id, long long dim, const long long* n, long long includePressure, long long nrows,
                                      const long long* rowptr, const long long* colA, const double* valA, long long VankaType, const double* w,
                                      long long nw, mg_vanka** out) {
  return vanka_create_built(true, device_id, dim, n, includePressure, nrows, rowptr, colA, valA, VankaType, w, nw, out);
}
// mg_vanka_build_blocks_*: the handle's blocks again from its resident operator; a singular cell leaves the previous blocks in place
int mg_vanka_build_blocks_FP64(mg_vanka* v, long long VankaType, const double* w, long long nw) {
  return vanka_build_entry(false, v, VankaType, w, nw, "mg_vanka_build_blocks_FP64");
}
int mg_vanka_build_blocks_CFP64(mg_vanka* v, long long VankaType, const double* w, long long nw) {
  return vanka_build_entry(true, v, VankaType, w, nw, "mg_vanka_build_blocks_CFP64");
}
// mg_vanka_replace_values_*: new values of the operator (valA's convention) on the stored pattern; the blocks are not touched
int mg_vanka_replace_values_FP64(mg_vanka* v, const double* nzval, long long nnz) {
  return vanka_replace_values(false, v, nzval, nnz, "mg_vanka_replace_values_FP64");
}
int mg_vanka_replace_values_CFP64(mg_vanka* v, const double* nzval, long long nnz) {
  return vanka_replace_values(true, v, nzval, nnz, "mg_vanka_replace_values_CFP64");
}
// mg_vanka_get_blocks: the handle's blocks as mg_vanka_create_* takes them; count = bs*bs*cells values (Float32, or ComplexF32 pairs)
int mg_vanka_get_blocks(mg_vanka* v, float* out, long long count) {
  if (!v || !out) return fail(MG_ERR_INVALID, "null argument");
  const long long want = (long long)v->core.G.bs * v->core.G.bs * v->core.G.cells;
  if (count != want) return fail(MG_ERR_INVALID, "count=%lld: the handle holds %lld block values", count, want);
  (void)hipSetDevice(v->device);
  HIP_TRY(spin_sync(v->stream));
  HIP_TRY(hipMemcpy(out, v->core.D.p, vanka_block_floats(&v->core) * sizeof(float), hipMemcpyDeviceToHost));
  return MG_OK;
}

// Measurement: device time of one build (into the spare buffer; the handle's blocks are not replaced), as mg_vanka_time_dev
int mg_vanka_time_build(mg_vanka* v, long long VankaType, const double* w, long long nw, long long warmup, long long reps, double* ms) {
  if (!v || !ms || reps < 1 || warmup < 0) return fail(MG_ERR_INVALID, "bad argument");
  mgk::VankaBuild P;
  MG_TRY(vanka_build_args(VankaType, w, nw, &P));
  (void)hipSetDevice(v->device);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = MG_OK;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) rc = fail(MG_ERR_HIP, "hipEventCreate failed");
  for (long long it = 0; it < warmup + reps && rc == MG_OK; ++it) {
    if (hipEventRecord(e0, v->stream) != hipSuccess) rc = fail(MG_ERR_HIP, "hipEventRecord failed");
    if (rc == MG_OK) rc = vanka_build_launch(&v->core, v->rowptr.p, v->col.p, v->val.p, P, v->stream);
    if (rc == MG_OK) {
      float t = 0.f;
      if (hipEventRecord(e1, v->stream) != hipSuccess || spin_sync(v->stream) != hipSuccess || hipEventElapsedTime(&t, e0, e1) != hipSuccess)
        rc = fail(MG_ERR_HIP, "event timing failed");
      if (it >= warmup) ms[it - warmup] = (double)t;
    }
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  return rc;
}

int mg_vanka_apply_FP64(mg_vanka* v, double* x, const double* b, long long numit, long long VankaType) {
  return vanka_apply_host(false, v, x, b, numit, VankaType, "mg_vanka_apply_FP64");
}
int mg_vanka_apply_CFP64(mg_vanka* v, double* x, const double* b, long long numit, long long VankaType) {
  return vanka_apply_host(true, v, x, b, numit, VankaType, "mg_vanka_apply_CFP64");
}
int mg_vanka_apply_dev_FP64(mg_vanka* v, double* x_dev, const double* b_dev, long long numit, long long VankaType) {
  return vanka_apply_dev(false, v, x_dev, b_dev, numit, VankaType, "mg_vanka_apply_dev_FP64");
}
int mg_vanka_apply_dev_CFP64(mg_vanka* v, double* x_dev, const double* b_dev, long long numit, long long VankaType) {
  return vanka_apply_dev(true, v, x_dev, b_dev, numit, VankaType, "mg_vanka_apply_dev_CFP64");
}

// The same on a block of nrhs right-hand sides (1..16; kernels: the _blk forms of mg_vanka.hpp).  Host forms: x, b column-major
// N x nrhs; _dev forms: row-major [N][nrhs] device blocks.  Column c holds the bits mg_vanka_apply_* gives on column c alone.
int mg_vanka_apply_block_FP64(mg_vanka* v, double* x, const double* b, long long nrhs, long long numit, long long VankaType) {
  return vanka_apply_block_host(false, v, x, b, nrhs, numit, VankaType, "mg_vanka_apply_block_FP64");
}
int mg_vanka_apply_block_CFP64(mg_vanka* v, double* x, const double* b, long long nrhs, long long numit, long long VankaType) {
  return vanka_apply_block_host(true, v, x, b, nrhs, numit, VankaType, "mg_vanka_apply_block_CFP64");
}
int mg_vanka_apply_block_dev_FP64(mg_vanka* v, double* x_dev, const double* b_dev, long long nrhs, long long numit, long long VankaType) {
  return vanka_apply_block_dev(false, v, x_dev, b_dev, nrhs, numit, VankaType, "mg_vanka_apply_block_dev_FP64");
}
int mg_vanka_apply_block_dev_CFP64(mg_vanka* v, double* x_dev, const double* b_dev, long long nrhs, long long numit, long long VankaType) {
  return vanka_apply_block_dev(true, v, x_dev, b_dev, nrhs, numit, VankaType, "mg_vanka_apply_block_dev_CFP64");
}

// Measurement: mg_vanka_time_dev on a row-major device block of nrhs columns
int mg_vanka_time_block_dev(mg_vanka* v, double* x_dev, const double* b_dev, long long nrhs, long long VankaType, long long warmup,
                            long long reps, double* ms) {
  if (!v || !ms || reps < 1 || warmup < 0) return fail(MG_ERR_INVALID, "bad argument");
  MG_TRY(vanka_block_args(v->core.cx, v, x_dev, b_dev, nrhs, 1, VankaType, "mg_vanka_time_block_dev"));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = MG_OK;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) rc = fail(MG_ERR_HIP, "hipEventCreate failed");
  for (long long it = 0; it < warmup + reps && rc == MG_OK; ++it) {
    if (hipEventRecord(e0, v->stream) != hipSuccess) rc = fail(MG_ERR_HIP, "hipEventRecord failed");
    if (rc == MG_OK) rc = vanka_run_blk(&v->core, v->rowptr.p, v->col.p, v->val.p, b_dev, x_dev, (int)nrhs, 1, (int)VankaType, v->stream);
    if (rc == MG_OK) {
      float t = 0.f;
      if (hipEventRecord(e1, v->stream) != hipSuccess || spin_sync(v->stream) != hipSuccess || hipEventElapsedTime(&t, e0, e1) != hipSuccess)
        rc = fail(MG_ERR_HIP, "event timing failed");
      if (it >= warmup) ms[it - warmup] = (double)t;
    }
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  return rc;
}

// info[0..8): value type (0 Float64, 1 ComplexF64); blockSize; cells; colours (2^dim); kernel launches of one
// FULL_VANKA_RB / ECON_VANKA_RB iteration (two per colour that holds a cell); of one FULL_VANKA_ADD iteration (one, plus one
// per call for the deltas); unknowns; kernels this handle has enqueued so far
int mg_vanka_info(mg_vanka* v, long long* info) {
  if (!v || !info) return fail(MG_ERR_INVALID, "null argument");
  info[0] = v->core.cx ? 1 : 0;
  info[1] = v->core.G.bs;
  info[2] = v->core.G.cells;
  info[3] = 1LL << v->core.G.dim;
  info[4] = 2LL * v->core.colours_live;
  info[5] = 1;
  info[6] = v->core.G.N;
  info[7] = v->core.launches;
  return MG_OK;
}

// Measurement: device time of one iteration on device vectors, as mg_dd_time_dev measures a sweep - `warmup` untimed
// iterations, then `reps`, each between two events on the handle's stream; ms[0..reps) in milliseconds.  x is relaxed in place.
int mg_vanka_time_dev(mg_vanka* v, double* x_dev, const double* b_dev, long long VankaType, long long warmup, long long reps, double* ms) {
  if (!v || !ms || reps < 1 || warmup < 0) return fail(MG_ERR_INVALID, "bad argument");
  MG_TRY(vanka_args(v->core.cx, v, x_dev, b_dev, 1, VankaType, "mg_vanka_time_dev"));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = MG_OK;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) rc = fail(MG_ERR_HIP, "hipEventCreate failed");
  for (long long it = 0; it < warmup + reps && rc == MG_OK; ++it) {
    if (hipEventRecord(e0, v->stream) != hipSuccess) rc = fail(MG_ERR_HIP, "hipEventRecord failed");
    if (rc == MG_OK) rc = vanka_run(&v->core, v->rowptr.p, v->col.p, v->val.p, b_dev, x_dev, 1, (int)VankaType, v->stream);
    if (rc == MG_OK) {
      float t = 0.f;
      if (hipEventRecord(e1, v->stream) != hipSuccess || spin_sync(v->stream) != hipSuccess || hipEventElapsedTime(&t, e0, e1) != hipSuccess)
        rc = fail(MG_ERR_HIP, "event timing failed");
      if (it >= warmup) ms[it - warmup] = (double)t;
    }
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  return rc;
}

int mg_vanka_destroy(mg_vanka* v) {
  if (!v) return MG_OK;
  (void)hipSetDevice(v->device);
  if (v->stream) {
    (void)spin_sync(v->stream);
    (void)hipStreamDestroy(v->stream);
  }
  v->core.release();
  v->rowptr.release();
  v->col.release();
  for (DevBuf<double>* b : {&v->val, &v->stage_x, &v->stage_b, &v->bstage_x, &v->bstage_b}) b->release();
  delete v;
  return MG_OK;
}

}  // extern "C"
