// mg_transport.inc - part of libmgvcycle.so's single translation unit (included by mgvcycle.hip in this order; not compiled on its own).
// The transport of both sharded forms (mg_ghost_* and mg_dist_*): the one place that talks to RCCL and to the host-staged plug-in.
// A handle holds one Transport by value; which transport it uses is decided where the communicator, the plug-in or the dry flag is
// set, and every collective (peer exchange by splits, all-reduce of doubles, all-gather) runs on it from here.
namespace {
// RCCL is loaded lazily (dlopen) so that single-GPU users of the library do not depend on it.
// Prototypes, handle types and enumerators come from the RCCL header this library is built against (rccl/rccl.h):
// decltype(&ncclSend) etc. - if the ABI moves, the build follows it or fails, it cannot go silently wrong.
struct Rccl {
  typedef ncclUniqueId UniqueId;
  void* lib = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclCommCount) CommCount = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclSend) Send = nullptr;
  decltype(&ncclRecv) Recv = nullptr;
  decltype(&ncclAllReduce) AllReduce = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  bool load() {
    if (lib) return true;
    for (const char* name : {"librccl.so.1", "librccl.so"}) {
      lib = dlopen(name, RTLD_NOW | RTLD_NOLOAD);          // the copy torch already mapped, if any
      if (!lib) lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (lib) break;
    }
    if (!lib) return false;
    auto sym = [&](const char* n) { return dlsym(lib, n); };
    GetUniqueId = reinterpret_cast<decltype(GetUniqueId)>(sym("ncclGetUniqueId"));
    CommInitRank = reinterpret_cast<decltype(CommInitRank)>(sym("ncclCommInitRank"));
    CommDestroy = reinterpret_cast<decltype(CommDestroy)>(sym("ncclCommDestroy"));
    CommCount = reinterpret_cast<decltype(CommCount)>(sym("ncclCommCount"));
    GroupStart = reinterpret_cast<decltype(GroupStart)>(sym("ncclGroupStart"));
    GroupEnd = reinterpret_cast<decltype(GroupEnd)>(sym("ncclGroupEnd"));
    Send = reinterpret_cast<decltype(Send)>(sym("ncclSend"));
    Recv = reinterpret_cast<decltype(Recv)>(sym("ncclRecv"));
    AllReduce = reinterpret_cast<decltype(AllReduce)>(sym("ncclAllReduce"));
    AllGather = reinterpret_cast<decltype(AllGather)>(sym("ncclAllGather"));
    GetErrorString = reinterpret_cast<decltype(GetErrorString)>(sym("ncclGetErrorString"));
    return GetUniqueId && CommInitRank && CommDestroy && GroupStart && GroupEnd && Send && Recv && AllReduce && AllGather;
  }
};
Rccl g_rccl;
constexpr ncclDataType_t NCCL_DOUBLE = ncclFloat64;
constexpr ncclRedOp_t NCCL_SUM = ncclSum;
static_assert(sizeof(ncclUniqueId) == 128, "mg_dist_unique_id / mg_dist_create exchange the RCCL id as 128 bytes");
static_assert(ncclFloat64 == 8 && ncclSum == 0, "RCCL enumerators moved: check the glue in INTEGRATION.md");

int dist_nccl(ncclResult_t rc, const char* what) {
  if (rc == ncclSuccess) return MG_OK;
  return fail(MG_ERR_HIP, "%s failed: %s", what, g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "RCCL error");
}
#define NCCL_TRY(expr) MG_TRY(dist_nccl((expr), #expr))

struct Transport {
  // NONE: nothing to talk to (a world of one without a communicator; a larger world before its transport is set - ready() refuses it)
  // RCCL: collectives are enqueued on the caller's stream      PLUGIN: host-staged through `plug`, done on return
  // DRY:  one rank of a larger world alone on its GPU (timing aid): nothing travels, sums stay local
  enum Mode { NONE, RCCL, PLUGIN, DRY };
  struct Pair { const double* send; double* recv; };   // device buffers of a peer exchange, each laid out peer by peer

  int rank = 0, world = 1;
  Mode mode = NONE;
  ncclComm_t comm = nullptr;            // the collectives on the compute stream
  ncclComm_t comm_side = nullptr;       // optional second communicator for exchanges on a side stream: operations on ONE communicator are
                                        // serialised in issue order whatever their streams (init_side)
  mg_exchange_fn plug = nullptr;        // host-staged transport (tests / ranks sharing one GPU)
  void* plug_user = nullptr;
  bool dry = false;
  double* h_stage = nullptr;            // pinned staging of the plug-in's collectives, grow-only (stage)
  size_t h_stage_n = 0;
  long long n_exchanges = 0, n_sent = 0, n_allreduce = 0;   // peer exchanges started, doubles sent, all-reduces entered by this rank

  void derive() { mode = comm ? RCCL : world <= 1 ? NONE : dry ? DRY : plug ? PLUGIN : NONE; }
  // transfers run on the stream they are given (the caller may go on and wait for an event), not on the host before the call returns
  bool on_stream() const { return mode == RCCL; }
  // sums are taken over the owned rows of a partition (also a world of one going through RCCL, as the sharded bench does)
  bool sharded() const { return mode != NONE; }
  // a sum really comes back added over all `world` ranks
  bool sums_global() const { return mode == RCCL || mode == PLUGIN; }

  int init_comm(ncclComm_t* c, const char* id128) {
    if (!g_rccl.load()) return fail(MG_ERR_HIP, "librccl.so could not be loaded");
    Rccl::UniqueId u;
    std::memcpy(u.internal, id128, 128);
    MG_TRY(dist_nccl(g_rccl.CommInitRank(c, world, u, rank), "ncclCommInitRank"));
    derive();
    return MG_OK;
  }
  int init_rccl(const char* id128) { return init_comm(&comm, id128); }
  int init_side(const char* id128) {
    if (!comm) return fail(MG_ERR_STATE, "this handle was created without an RCCL communicator");
    if (comm_side) return fail(MG_ERR_STATE, "the side communicator is already set");
    return init_comm(&comm_side, id128);
  }
  int set_plugin(mg_exchange_fn fn, void* user) {
    if (!fn) return fail(MG_ERR_INVALID, "null argument");
    if (comm) return fail(MG_ERR_STATE, "this handle was created with an RCCL communicator");
    plug = fn;
    plug_user = user;
    derive();
    return MG_OK;
  }
  int set_dry(bool on) {
    if (comm) return fail(MG_ERR_STATE, "this handle was created with an RCCL communicator");
    dry = on;
    derive();
    return MG_OK;
  }
  int ready() const {
    if (world > 1 && mode == NONE) return fail(MG_ERR_STATE, "no transport: pass an RCCL unique id when the handle is created or set an exchange plug-in");
    return MG_OK;
  }
  // ranks of the communicator AS RCCL REPORTS THEM (ncclCommCount); 0 without one
  int comm_count(long long* count) const {
    *count = 0;
    if (!comm) return MG_OK;
    if (!g_rccl.CommCount) return fail(MG_ERR_UNSUPPORTED, "this librccl has no ncclCommCount");
    int c = 0;
    NCCL_TRY(g_rccl.CommCount(comm, &c));
    *count = c;
    return MG_OK;
  }
  // (the caller has drained its streams)
  void release() {
    if (comm_side && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(comm_side);
    if (comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(comm);
    if (h_stage) (void)hipHostFree(h_stage);
    comm = comm_side = nullptr;
    h_stage = nullptr;
    h_stage_n = 0;
    derive();
  }

  // at least n pinned doubles in h_stage.  Growing frees the old block, which a copy enqueued earlier on s (the upload at the end of a
  // plug-in collective) may still read: s is drained first.
  int stage(size_t n, hipStream_t s) {
    if (h_stage_n >= n) return MG_OK;
    HIP_TRY(spin_sync(s));
    if (h_stage) (void)hipHostFree(h_stage);
    h_stage = nullptr;
    h_stage_n = 0;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_stage), sizeof(double) * n));
    h_stage_n = n;
    return MG_OK;
  }

  // ---- all-reduce (sum) of n doubles ----
  // v (device) <- its sum over the ranks; nothing waits for the host on RCCL
  int allreduce_dev(double* v, size_t n, hipStream_t s) {
    if (mode == RCCL) {
      NCCL_TRY(g_rccl.AllReduce(v, v, n, NCCL_DOUBLE, NCCL_SUM, comm, s));
      ++n_allreduce;
    } else if (mode == PLUGIN) {
      MG_TRY(stage(n, s));
      MG_TRY(allreduce_now(v, n, h_stage, s));
      HIP_TRY(hipMemcpyAsync(v, h_stage, sizeof(double) * n, hipMemcpyHostToDevice, s));
    }
    return MG_OK;
  }
  // Split form: start enqueues the all-reduce of v (RCCL, in place) and its copy into `slot` (pinned, the caller's); once what start
  // enqueued has run, finish adds the ranks' sums where the plug-in does that (op 1) - the slot then holds the global sum in every mode.
  // finish touches no staging: the stream may already hold later work (the solve loop reads step k's norm behind step k+1).
  int allreduce_start(double* v, size_t n, double* slot, hipStream_t s) {
    if (mode == RCCL) {
      NCCL_TRY(g_rccl.AllReduce(v, v, n, NCCL_DOUBLE, NCCL_SUM, comm, s));
      ++n_allreduce;
    }
    HIP_TRY(hipMemcpyAsync(slot, v, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    return MG_OK;
  }
  int allreduce_finish(double* slot, size_t n) {
    if (mode != PLUGIN) return MG_OK;
    const std::vector<double> in(slot, slot + n);
    if (plug(plug_user, 1, in.data(), nullptr, slot, nullptr, (long long)n) != 0) return fail(MG_ERR_HIP, "exchange plug-in failed (all_reduce)");
    ++n_allreduce;
    return MG_OK;
  }
  // slot (pinned) <- the sum over the ranks of v (device), on the host now: synchronises s
  int allreduce_now(double* v, size_t n, double* slot, hipStream_t s) {
    MG_TRY(allreduce_start(v, n, slot, s));
    HIP_TRY(spin_sync(s));
    return allreduce_finish(slot, n);
  }

  // ---- peer exchange ----
  // For each pair: k * send_splits[p] doubles of `send` go to peer p, k * recv_splits[p] doubles of `recv` come from it, peer by peer
  // in rank order (k: right-hand sides per row).  RCCL: one group of sends / receives for all pairs on s, on the side communicator
  // where asked for and set.  Plug-in: one all_to_all (op 0) per pair, s drained, the upload into `recv` enqueued on s.
  int exchange(const Pair* pairs, int npairs, const std::vector<long long>& send_splits, const std::vector<long long>& recv_splits, long long k,
               hipStream_t s, bool side_comm = false) {
    long long n_send = 0, n_recv = 0;
    for (int p = 0; p < world; ++p) { n_send += send_splits[(size_t)p] * k; n_recv += recv_splits[(size_t)p] * k; }
    ++n_exchanges;
    n_sent += n_send * npairs;
    if (mode == RCCL) {
      ncclComm_t c = (side_comm && comm_side) ? comm_side : comm;
      NCCL_TRY(g_rccl.GroupStart());
      long long so = 0, ro = 0;
      for (int peer = 0; peer < world; ++peer) {
        const long long ns = send_splits[(size_t)peer] * k, nr = recv_splits[(size_t)peer] * k;
        for (int q = 0; q < npairs; ++q) {
          if (ns > 0) NCCL_TRY(g_rccl.Send(pairs[q].send + so, (size_t)ns, NCCL_DOUBLE, peer, c, s));
          if (nr > 0) NCCL_TRY(g_rccl.Recv(pairs[q].recv + ro, (size_t)nr, NCCL_DOUBLE, peer, c, s));
        }
        so += ns;
        ro += nr;
      }
      NCCL_TRY(g_rccl.GroupEnd());
    } else if (mode == PLUGIN) {
      std::vector<long long> ss(send_splits), rs(recv_splits);   // (counts in doubles: rows x right-hand sides)
      for (auto& c : ss) c *= k;
      for (auto& c : rs) c *= k;
      MG_TRY(stage((size_t)(n_send + n_recv) + 1, s));   // (+ 1: never a null buffer for the plug-in, whatever the splits)
      double *hs = h_stage, *hr = h_stage + n_send;
      for (int q = 0; q < npairs; ++q) {
        if (n_send > 0) HIP_TRY(hipMemcpyAsync(hs, pairs[q].send, sizeof(double) * (size_t)n_send, hipMemcpyDeviceToHost, s));
        HIP_TRY(spin_sync(s));   // (also: the previous pair's upload has left the staging)
        if (plug(plug_user, 0, hs, ss.data(), hr, rs.data(), 0) != 0) return fail(MG_ERR_HIP, "exchange plug-in failed (all_to_all)");
        if (n_recv > 0) HIP_TRY(hipMemcpyAsync(pairs[q].recv, hr, sizeof(double) * (size_t)n_recv, hipMemcpyHostToDevice, s));
      }
    } else if (mode != DRY) {
      return fail(MG_ERR_STATE, "a peer exchange on a handle without a transport");
    }
    return MG_OK;
  }

  // ---- all-gather: recv (device, world x count) <- every rank's send (device, count), in rank order ----
  int allgather(const double* send, double* recv, size_t count, hipStream_t s) {
    if (mode == RCCL) {
      NCCL_TRY(g_rccl.AllGather(send, recv, count, NCCL_DOUBLE, comm, s));
    } else if (mode == PLUGIN) {
      MG_TRY(stage(count * (size_t)(world + 1), s));
      HIP_TRY(hipMemcpyAsync(h_stage, send, sizeof(double) * count, hipMemcpyDeviceToHost, s));
      HIP_TRY(spin_sync(s));
      if (plug(plug_user, 2, h_stage, nullptr, h_stage + count, nullptr, (long long)count) != 0) return fail(MG_ERR_HIP, "exchange plug-in failed (all_gather)");
      HIP_TRY(hipMemcpyAsync(recv, h_stage + count, sizeof(double) * count * (size_t)world, hipMemcpyHostToDevice, s));
    } else {
      HIP_TRY(hipMemcpyAsync(recv, send, sizeof(double) * count, hipMemcpyDeviceToDevice, s));
    }
    return MG_OK;
  }
};
}  // namespace
