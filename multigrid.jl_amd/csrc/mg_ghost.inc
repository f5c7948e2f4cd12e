// mg_ghost.inc - part of libmgvcycle.so's single translation unit (included by mgvcycle.hip in this order; not compiled on its own).
// Sharded cycle with deep ghost layers (mg_ghost_*): a rank's hierarchy is an ordinary mg_hierarchy on its box EXTENDED by ghost
// layers; this part owns the exchange of those layers (packing, streams and events; the wire is mg_transport.inc), the validity
// bookkeeping that decides when an exchange is due, the all-reduce into the first replicated level and the global norms.
// Reference: the `overlap` of src/DomainDecomposition/DDIndices.jl:61-92 (box rule l.41-47), fan-out DDParallel.jl:87-105,133-139.
namespace {
constexpr int GH_FULL = 1 << 20;   // validity depth of a vector whose every ghost layer is up to date

struct GhostLevel {
  bool set = false, active = false;     // active: some rank exchanges something on this level (a collective is entered by all or none)
  int ext[3] = {1, 1, 1}, lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};   // extended box; owned box [lo, hi) inside it
  int gmin = GH_FULL;                   // smallest ghost width over the cut sides
  long long n = 0, n_send = 0, n_recv = 0;
  DevBuf<int> send_idx, recv_idx;
  DevBuf<double> send_buf, recv_buf, send_buf2, recv_buf2;   // (…2: the second vector of a two-vector exchange)
  std::vector<long long> send_splits, recv_splits;
  const double* pending2 = nullptr;                  // second vector of the exchange in flight
  hipEvent_t ev_packed = nullptr, ev_landed = nullptr;
  std::vector<std::pair<const double*, int>> depth;  // validity depth of the level's vectors (by address)
  const double* pending = nullptr;                   // vector whose ghost layers are in flight on the side stream
  DevBuf<double> send_blk, recv_blk;                 // a BLOCK's ghost layers (row-major [n][k]; the sharded block Krylov drivers)
};
}  // namespace

struct mg_ghost {
  int a = 0;                            // sharded levels (0 .. a-1 live on extended boxes, a .. are replicated)
  Transport T;                          // all-reduces on its communicator, the ghost-layer send / recv of the side stream on its side communicator: the
                                        // fine level's exchange would else sit in front of the next all-reduce instead of beside the coarse cycle
  hipStream_t side = nullptr;
  std::vector<GhostLevel> lev;
  DevBuf<double> b0;                    // the fine right-hand side with its ghost layers (the caller's b is read-only)
  double* h_norm = nullptr;             // pinned scalar of gh_norm_own
  DevBuf<double> kscal;                 // scalars of the sharded Krylov drivers (gh_dots_own), all-reduced in place
  double* h_kscal = nullptr;            // ... and their pinned mirror
  bool finalized = false;
  // What the kernels of a level can do decides where exchanges happen, and EVERY rank must take the same decisions (a collective is
  // entered by all or none): the boxes of two ranks differ by a line or two, so a format builder may serve one and not the other.
  // mg_ghost_finalize adds the ranks' 0/1 flags up (one all-reduce) and keeps a capability only where all `world` ranks have it.
  bool agree4 = true;                   // level 1: the four-stage pass (march4_ok)
  std::vector<char> agree2, agree_zero, agree_scale;   // per sharded level: the fused sweep + residual, its from-zero form, d.*bc out of the restriction
  bool bad_depth = false;               // an operation consumed more ghost layers than its input had (gh_set with a negative depth): the
                                        // results next to the cut are wrong - every later exchange and the end of the call report MG_ERR_STATE
};

namespace {
inline GhostLevel* gh_level(const mg_hierarchy* h, int l) {
  mg_ghost* g = h->ghost;
  if (!g || !g->finalized || l < 0 || l >= g->a) return nullptr;
  GhostLevel& L = g->lev[(size_t)l];
  return L.active ? &L : nullptr;
}
// the box of rows whose r^2 counts on `level`: the owned box where the level lives on an extended box, else untouched
void gh_own_box(const mg_hierarchy* h, int level, int* xl, int* xh, int* yl, int* yh, int* zl, int* zh) {
  GhostLevel* L = gh_level(h, level);
  if (!L) return;
  *xl = L->lo[0]; *xh = L->hi[0]; *yl = L->lo[1]; *yh = L->hi[1]; *zl = L->lo[2]; *zh = L->hi[2];
}
// norms are sums over several ranks (or go through RCCL at a world of one, as the sharded bench does)
bool gh_global_scalars(const mg_hierarchy* h) { return h->ghost && h->ghost->finalized && h->ghost->T.sharded(); }
inline bool gh_agree2(const mg_hierarchy* h, int l) { return !h->ghost || !h->ghost->finalized || l >= h->ghost->a || h->ghost->agree2[(size_t)l]; }
inline bool gh_agree_zero(const mg_hierarchy* h, int l) { return !h->ghost || !h->ghost->finalized || l >= h->ghost->a || h->ghost->agree_zero[(size_t)l]; }
inline bool gh_agree_scale(const mg_hierarchy* h, int l) { return !h->ghost || !h->ghost->finalized || l >= h->ghost->a || h->ghost->agree_scale[(size_t)l]; }
inline bool gh_agree4(const mg_hierarchy* h) { return !h->ghost || !h->ghost->finalized || h->ghost->agree4; }
// ---- validity bookkeeping ------------------------------------------------------------------------------------------------------
// depth(v) = v is valid on the owned box grown by that many layers towards the cut sides (GH_FULL: every ghost layer).  A product
// with A (radius 1 on every level: 7-point fine, 27-point Galerkin) costs one layer; a vector with every layer valid gives a result
// valid on gmin - 1 (the outermost layer of the extended box holds rows cut off at the artificial boundary).
inline int gh_depth(const mg_hierarchy* h, int l, const double* v) {
  GhostLevel* L = gh_level(h, l);
  if (!L) return GH_FULL;
  for (auto& e : L->depth)
    if (e.first == v) return e.second;
  return 0;   // (a vector nobody recorded: the owned rows are all that may be assumed)
}
inline void gh_set(mg_hierarchy* h, int l, const double* v, int d) {
  GhostLevel* L = gh_level(h, l);
  if (!L || !v) return;
  if (d >= L->gmin) d = GH_FULL;
  if (d < 0) {      // (a pass deeper than the level's ghost width was launched: a schedule bug, never clamped silently - ADVICE r5)
    h->ghost->bad_depth = true;
    d = 0;
  }
  for (auto& e : L->depth)
    if (e.first == v) { e.second = d; return; }
  L->depth.emplace_back(v, d);
}
inline int gh_dec(const mg_hierarchy* h, int l, int d) {
  GhostLevel* L = gh_level(h, l);
  if (!L) return GH_FULL;
  return d >= GH_FULL ? L->gmin - 1 : d - 1;
}

int gh_check_depths(const mg_hierarchy* h) {
  if (h->ghost && h->ghost->bad_depth)
    return fail(MG_ERR_STATE, "ghost-layer form: a pass consumed more ghost layers than its input was valid on (rows next to the cut are wrong)");
  return MG_OK;
}
int gh_exchange_finish(mg_hierarchy* h, int l) {
  GhostLevel* L = gh_level(h, l);
  if (!L || !L->pending) return MG_OK;
  HIP_TRY(hipStreamWaitEvent(h->play->stream, L->ev_landed, 0));   // (pending: the exchange went over the side stream)
  L->pending = nullptr;
  L->pending2 = nullptr;
  return MG_OK;
}
// Refresh every ghost layer of v from the ranks that own those nodes (v valid on the owned box).  RCCL: the values the peers
// need are packed on the compute stream, sent / received and put in place on the SIDE stream; the compute stream goes on and waits
// for the landing (gh_exchange_finish) in front of the first kernel that touches v.  Plug-in: done on return.
// v2 (optional): a second vector of the same level travels in the same exchange (one pack, one group of sends / receives, one unpack)
// side: the caller goes on with other work and waits later (gh_prefetch: the fine level's exchange beside the coarse cycle) - send / receive
// and unpack run on the SIDE stream; else the exchange is awaited at once and everything stays on the compute stream: a hop to another
// stream and back costs two cross-stream waits (measured in the dry run: ~20 us per exchange, more than the small levels' exchanges take)
int gh_exchange_start(mg_hierarchy* h, int l, double* v, double* v2 = nullptr, bool side = false) {
  GhostLevel* L = gh_level(h, l);
  if (!L) return MG_OK;
  mg_ghost* g = h->ghost;
  if (h->capturing) return fail(MG_ERR_STATE, "a ghost-layer exchange inside a graph capture");
  MG_TRY(gh_check_depths(h));
  MG_TRY(gh_exchange_finish(h, l));   // (one exchange in flight per level: the send buffer is free again)
  ProfScope ps(h, l, MG_K_GHOST, (v2 ? 40.0 : 20.0) * (double)(L->n_send + L->n_recv));
  const unsigned nbs = (unsigned)((L->n_send + mgk::BLK - 1) / mgk::BLK), nbr = (unsigned)((L->n_recv + mgk::BLK - 1) / mgk::BLK);
  auto unpack = [&](hipStream_t st) {
    if (L->n_recv <= 0) return;
    if (v2) hipLaunchKernelGGL(mgk::ghost_unpack2, dim3(nbr), dim3(mgk::BLK), 0, st, L->recv_buf.p, L->recv_buf2.p, L->recv_idx.p, v, v2, L->n_recv);
    else hipLaunchKernelGGL(mgk::ghost_unpack, dim3(nbr), dim3(mgk::BLK), 0, st, L->recv_buf.p, L->recv_idx.p, v, L->n_recv);
  };
  if (L->n_send > 0) {
    if (v2) hipLaunchKernelGGL(mgk::ghost_pack2, dim3(nbs), dim3(mgk::BLK), 0, h->play->stream, v, v2, L->send_idx.p, L->send_buf.p, L->send_buf2.p, L->n_send);
    else hipLaunchKernelGGL(mgk::ghost_pack, dim3(nbs), dim3(mgk::BLK), 0, h->play->stream, v, L->send_idx.p, L->send_buf.p, L->n_send);
  }
  HIP_TRY(hipGetLastError());
  // (the hop needs a wire to wait for.  Dry, nothing travels: pack and unpack on the compute stream.  Measured, round 6: the unpack of the
  // fine level's prefetch on the side stream - the RCCL transport's structure - costs the dry rank 26 us MORE than the 19 us of kernel time it
  // moves out of the way: 0.5693 against 0.543 ms per step; with a wire to wait for the hop pays, without one it does not.)
  const bool hop = side && g->T.on_stream();
  hipStream_t xs = hop ? g->side : h->play->stream;
  if (hop) {
    HIP_TRY(hipEventRecord(L->ev_packed, h->play->stream));
    HIP_TRY(hipStreamWaitEvent(g->side, L->ev_packed, 0));
  }
  const Transport::Pair pairs[2] = {{L->send_buf.p, L->recv_buf.p}, {L->send_buf2.p, L->recv_buf2.p}};
  MG_TRY(g->T.exchange(pairs, v2 ? 2 : 1, L->send_splits, L->recv_splits, 1, xs, /*side_comm=*/hop));
  unpack(xs);
  HIP_TRY(hipGetLastError());
  if (hop) {
    HIP_TRY(hipEventRecord(L->ev_landed, g->side));
    L->pending = v;
    L->pending2 = v2;
  }
  gh_set(h, l, v, GH_FULL);
  if (v2) gh_set(h, l, v2, GH_FULL);
  return MG_OK;
}
// v is about to be read or written by a kernel on the compute stream: an exchange of it that is still in flight lands first
inline int gh_touch(mg_hierarchy* h, int l, const double* v) {
  GhostLevel* L = gh_level(h, l);
  if (L && L->pending && (L->pending == v || L->pending2 == v)) return gh_exchange_finish(h, l);
  return MG_OK;
}
// the next operation needs v valid on `want` layers: exchange (and wait) if it is not
int gh_need(mg_hierarchy* h, int l, const double* v, int want) {
  GhostLevel* L = gh_level(h, l);
  if (!L) return MG_OK;
  if (gh_depth(h, l, v) < std::min(want, L->gmin)) {
    MG_TRY(gh_touch(h, l, v));
    MG_TRY(gh_exchange_start(h, l, const_cast<double*>(v)));
    return gh_exchange_finish(h, l);
  }
  return gh_touch(h, l, v);
}
// the operation `want` layers deep is some launches away: start the exchange now if v will not do, wait for it later (gh_need / gh_touch)
int gh_prefetch(mg_hierarchy* h, int l, double* v, int want) {
  GhostLevel* L = gh_level(h, l);
  if (!L) return MG_OK;
  if (gh_depth(h, l, v) < std::min(want, L->gmin)) return gh_exchange_start(h, l, v, nullptr, /*side=*/true);
  return MG_OK;
}

// ---- into the first replicated level: bc (one row per node of that level, non-zero where this rank owns the node) summed over the ranks ----
int gh_allreduce_tail(mg_hierarchy* h, double* v, long long n) {
  mg_ghost* g = h->ghost;
  if (!g || !g->finalized) return MG_OK;
  if (h->capturing && g->T.on_stream()) return fail(MG_ERR_STATE, "an all-reduce inside a graph capture");
  return g->T.allreduce_dev(v, (size_t)n, h->play->stream);
}
// ---- global norms ------------------------------------------------------------------------------------------------------------------
// h->play->scalar holds this rank's sum of squares over its OWNED rows: all-reduce it on the stream (RCCL) and copy it into `slot` (pinned);
// with the plug-in the slot receives the local sum and gh_host_reduce adds the ranks' sums when the host reads it.
int gh_scalar_to_slot(mg_hierarchy* h, double* slot) { return h->ghost->T.allreduce_start(h->play->scalar.p, 1, slot, h->play->stream); }
int gh_host_reduce(mg_hierarchy* h, double* slot) { return h->ghost ? h->ghost->T.allreduce_finish(slot, 1) : MG_OK; }
// enqueue: *slot (pinned) <- sum of squares of v over the owned rows [of every rank: RCCL; with the plug-in the local sum, to be passed
// through gh_host_reduce once the stream has drained]
int gh_sumsq_own_to_slot(mg_hierarchy* h, const double* v, double* slot) {
  mg_ghost* g = h->ghost;
  const GhostLevel& L = g->lev[0];
  mgk::BoxDev B;
  B.n1 = L.ext[0]; B.n2 = L.ext[1]; B.n3 = L.ext[2];
  for (int k = 0; k < 3; ++k) { B.lo[k] = L.lo[k]; B.hi[k] = L.hi[k]; }
  const long long lines = (long long)(L.hi[1] - L.lo[1]) * (L.hi[2] - L.lo[2]);
  const int nb = (int)std::max<long long>(1, std::min<long long>(h->nred_blocks, (lines + 3) / 4));
  hipLaunchKernelGGL(mgk::sumsq_box_partial, dim3(nb), dim3(mgk::BLK), 0, h->play->stream, v, B, h->play->partial.p);
  hipLaunchKernelGGL(mgk::sum_final, dim3(1), dim3(mgk::BLK), 0, h->play->stream, h->play->partial.p, nb, h->play->scalar.p);
  HIP_TRY(hipGetLastError());
  return gh_scalar_to_slot(h, slot);
}
// sqrt of the sum of squares of v over the owned rows of every rank (the fine level; SolveFuncs.jl:15,20,30); synchronises
int gh_norm_own(mg_hierarchy* h, const double* v, double* out) {
  mg_ghost* g = h->ghost;
  MG_TRY(gh_sumsq_own_to_slot(h, v, g->h_norm));
  HIP_TRY(spin_sync(h->play->stream));
  MG_TRY(gh_host_reduce(h, g->h_norm));
  *out = std::sqrt(*g->h_norm);
  return MG_OK;
}
// ---- sharded Krylov drivers (mg_krylov.inc; solveCG_MG / solveBiCGSTAB_MG / solveGMRES_MG, SolveFuncs.jl:74-133) ----------------
// out[c] = x_c ' y_c over the owned rows of every rank, c < count <= 8: `count` box dots, ONE all-reduce of `count` doubles, one
// host synchronisation (the scalars that are due at the same point of an iteration travel together).
// level: the (sharded) level the vectors live on - 0 for the Krylov drivers, l for the FGMRES relaxation of level l (Jac-GMRES, K-cycle)
int gh_dots_own(mg_hierarchy* h, int count, const double* const* xs, const double* const* ys, double* out, int level = 0) {
  mg_ghost* g = h->ghost;
  if (count < 1 || count > 8) return fail(MG_ERR_INVALID, "gh_dots_own: 1 to 8 scalars");
  if (level < 0 || level >= g->a) return fail(MG_ERR_INVALID, "gh_dots_own: level %d is not sharded", level + 1);
  if (g->kscal.n < 8) MG_TRY(g->kscal.alloc(8));
  if (!g->h_kscal) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&g->h_kscal), 8 * sizeof(double)));
  const GhostLevel& L = g->lev[(size_t)level];
  mgk::BoxDev B;
  B.n1 = L.ext[0]; B.n2 = L.ext[1]; B.n3 = L.ext[2];
  for (int k = 0; k < 3; ++k) { B.lo[k] = L.lo[k]; B.hi[k] = L.hi[k]; }
  const long long lines = (long long)(L.hi[1] - L.lo[1]) * (L.hi[2] - L.lo[2]);
  const int nb = (int)std::max<long long>(1, std::min<long long>(h->nred_blocks / 8, (lines + 3) / 4));
  for (int c = 0; c < count; ++c) {
    hipLaunchKernelGGL(mgk::dot_box_partial, dim3(nb), dim3(mgk::BLK), 0, h->play->stream, xs[c], ys[c], B, h->play->partial.p + (size_t)c * nb);
    hipLaunchKernelGGL(mgk::sum_final, dim3(1), dim3(mgk::BLK), 0, h->play->stream, h->play->partial.p + (size_t)c * nb, nb, g->kscal.p + c);
  }
  HIP_TRY(hipGetLastError());
  MG_TRY(g->T.allreduce_now(g->kscal.p, (size_t)count, g->h_kscal, h->play->stream));
  for (int c = 0; c < count; ++c) out[c] = g->h_kscal[c];
  return MG_OK;
}
// ---- blocks of right-hand sides (sharded block Krylov drivers: blockCG / blockBiCGSTB / blockFGMRES, SolveFuncs.jl:95,113,130) -----------
// every ghost layer of the fine-level block V ([n_ext][k] row-major, owned rows valid) from the ranks that own those rows; awaited at once
int gh_exchange_block(mg_hierarchy* h, double* V, int k) {
  GhostLevel* L = gh_level(h, 0);
  if (!L) return MG_OK;
  mg_ghost* g = h->ghost;
  if (h->capturing) return fail(MG_ERR_STATE, "a ghost-layer exchange inside a graph capture");
  MG_TRY(gh_exchange_finish(h, 0));
  const size_t ns = (size_t)std::max<long long>(L->n_send, 1) * (size_t)k, nr = (size_t)std::max<long long>(L->n_recv, 1) * (size_t)k;
  if (L->send_blk.n < ns) MG_TRY(L->send_blk.alloc(ns));
  if (L->recv_blk.n < nr) MG_TRY(L->recv_blk.alloc(nr));
  ProfScope ps(h, 0, MG_K_GHOST, 20.0 * (double)k * (double)(L->n_send + L->n_recv));
  if (L->n_send > 0)
    hipLaunchKernelGGL(mgk::ghost_pack_block, dim3((unsigned)((L->n_send * k + mgk::BLK - 1) / mgk::BLK)), dim3(mgk::BLK), 0, h->play->stream, V, L->send_idx.p, L->send_blk.p, L->n_send, k);
  HIP_TRY(hipGetLastError());
  const Transport::Pair pair = {L->send_blk.p, L->recv_blk.p};
  MG_TRY(g->T.exchange(&pair, 1, L->send_splits, L->recv_splits, k, h->play->stream));
  if (L->n_recv > 0)
    hipLaunchKernelGGL(mgk::ghost_unpack_block, dim3((unsigned)((L->n_recv * k + mgk::BLK - 1) / mgk::BLK)), dim3(mgk::BLK), 0, h->play->stream, L->recv_blk.p, L->recv_idx.p, V, L->n_recv, k);
  HIP_TRY(hipGetLastError());
  return MG_OK;
}
// G = X'Y (k x k, row-major, host) over the owned rows of every rank: box Gram + ONE all-reduce of k*k doubles; synchronises
int gh_gram_own(mg_hierarchy* h, const double* X, const double* Y, int k, double* G, DevBuf<double>& partial) {
  mg_ghost* g = h->ghost;
  const GhostLevel& L = g->lev[0];
  mgk::BoxDev B;
  B.n1 = L.ext[0]; B.n2 = L.ext[1]; B.n3 = L.ext[2];
  for (int q = 0; q < 3; ++q) { B.lo[q] = L.lo[q]; B.hi[q] = L.hi[q]; }
  const long long nown = (long long)(L.hi[0] - L.lo[0]) * (L.hi[1] - L.lo[1]) * (L.hi[2] - L.lo[2]);
  const int nb = (int)std::min<long long>(256, std::max<long long>(1, (nown + mgk::BLK - 1) / mgk::BLK));
  const size_t kk = (size_t)k * k;
  if (partial.n < (size_t)nb * kk + kk) MG_TRY(partial.alloc((size_t)nb * kk + kk));
  double* out = partial.p + (size_t)nb * kk;
  hipLaunchKernelGGL(mgk::blk_gram_box_partial, dim3(nb, k), dim3(mgk::BLK), 0, h->play->stream, X, Y, B, k, partial.p);
  hipLaunchKernelGGL(mgk::blk_gram_final, dim3(1), dim3(mgk::BLK), 0, h->play->stream, partial.p, nb, k, out);
  HIP_TRY(hipGetLastError());
  MG_TRY(g->T.stage(kk, h->play->stream));
  MG_TRY(g->T.allreduce_now(out, kk, g->T.h_stage, h->play->stream));
  std::memcpy(G, g->T.h_stage, sizeof(double) * kk);
  return MG_OK;
}
// every ghost layer of the fine-level vector v from its owners (v valid on the owned rows): what a product with A needs of its input
int gh_refresh(mg_hierarchy* h, double* v, int level = 0) {
  if (!gh_level(h, level)) return MG_OK;
  gh_set(h, level, v, 0);
  return gh_need(h, level, v, 1);
}
// is level l one whose sums run over the owned rows of all ranks (a sharded level of a ghost-attached handle)?
bool gh_sharded_sums(const mg_hierarchy* h, int l) { return gh_global_scalars(h) && l < h->ghost->a; }
// Start of a cycle / solve on one rank's extended boxes: the bookkeeping starts from "owned rows only", and b - read-only for the
// library - is copied into a buffer of the handle whose ghost layers are then filled (once per call: b does not change).
int gh_begin(mg_hierarchy* h, const double** b, double* x, bool x_zero) {
  mg_ghost* g = h->ghost;
  if (!g || !g->finalized) return MG_OK;
  g->bad_depth = false;
  for (int l = 0; l < g->a; ++l) {
    MG_TRY(gh_exchange_finish(h, l));
    g->lev[(size_t)l].depth.clear();
  }
  if (!gh_level(h, 0)) return MG_OK;
  HIP_TRY(hipMemcpyAsync(g->b0.p, *b, sizeof(double) * (size_t)g->lev[0].n, hipMemcpyDeviceToDevice, h->play->stream));
  gh_set(h, 0, g->b0.p, 0);
  MG_TRY(gh_need(h, 0, g->b0.p, GH_FULL));
  *b = g->b0.p;
  gh_set(h, 0, x, 0);
  (void)x_zero;
  return MG_OK;
}
// the same for a block solved column by column: the bookkeeping starts empty; the columns' ghost layers are the caller's to ask for
int gh_begin_block(mg_hierarchy* h) {
  mg_ghost* g = h->ghost;
  if (!g || !g->finalized) return MG_OK;
  g->bad_depth = false;
  for (int l = 0; l < g->a; ++l) {
    MG_TRY(gh_exchange_finish(h, l));
    g->lev[(size_t)l].depth.clear();
  }
  return MG_OK;
}
void gh_release(mg_ghost* g) {
  if (!g) return;
  if (g->side) (void)spin_sync(g->side);
  g->T.release();
  for (GhostLevel& L : g->lev) {
    L.send_idx.release(); L.recv_idx.release(); L.send_buf.release(); L.recv_buf.release(); L.send_buf2.release(); L.recv_buf2.release();
    L.send_blk.release(); L.recv_blk.release();
    if (L.ev_packed) (void)hipEventDestroy(L.ev_packed);
    if (L.ev_landed) (void)hipEventDestroy(L.ev_landed);
  }
  g->b0.release();
  if (g->h_norm) (void)hipHostFree(g->h_norm);
  if (g->h_kscal) (void)hipHostFree(g->h_kscal);
  g->kscal.release();
  if (g->side) (void)hipStreamDestroy(g->side);
  delete g;
}
}  // namespace
