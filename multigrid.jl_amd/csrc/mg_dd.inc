// mg_dd.inc - part of libmgvcycle.so's single translation unit (included by mgvcycle.hip; not compiled on its own).
// extern "C": the multiplicative Schwarz preconditioner of src/DomainDecomposition on the device (mg_dd_*):
// setupDDSerial's result (DDSerial.jl:81-106: index lists and one set of parLU factors per sub-domain) is uploaded once,
// mg_dd_apply_* runs solveDDSerial's sweeps (DDSerial.jl:108-139).  Kernels: mg_dd.hpp.
//
// Colour batching.  The reference walks the colours 1..2^dim and, inside a colour, the sub-domains in linear order.  Two
// members of a colour whose index sets are disjoint and whose listed rows store no column the other lists read and write
// disjoint parts of x: their order cannot be seen, and the whole colour is ONE launch (dd_color_sweep), factors of all
// sub-domains packed into shared arenas with one descriptor each.  A colour that fails the test (mg_dd_finalize checks it
// on the lists and the pattern, not on the geometry), or that holds a member of at least lu_multi_min_rows rows, runs its
// members one after another: residual gather, the factor applier's solve (single workgroup, or the chip-wide form of
// mg_lu_* for the large ones, as it is), scatter-add.  That is the reference's result in every case.
struct mg_dd {
  int device = 0;
  bool cx = false;                 // value type: false = FP64, true = CFP64
  long long n = 0, nnz = 0, numSub = 0;
  long long multi_min_rows = 0;    // lu_multi_min_rows, read once at create
  bool finalized = false;
  hipStream_t stream = nullptr;
  hipEvent_t ev_mine = nullptr, ev_theirs = nullptr;   // ordering against the stream of a member's own applier
  mg_hierarchy* owner = nullptr;   // mg_set_coarse_dd: the hierarchy that borrows this handle as its coarsest solve
  hipEvent_t ev_owner = nullptr;   // ... and the event that orders a stand-alone sweep behind that hierarchy's enqueued work
  DevBuf<int> rowptr, col, idx, members;
  DevBuf<double> val, r, y, w, stage_b, stage_x;
  struct Sub {
    long long n = 0, idx0 = 0;
    bool set = false;
    std::vector<long long> Lptr, Lcol, Uptr, Ucol, p, q;   // the caller's factors (1-based): the adjoint set is derived from them
    std::vector<double> Lval, Uval;
    mg_lu* big = nullptr;          // a member of >= multi_min_rows rows: an applier of its own (chip-wide form)
    long long big_launches = 0;
  };
  std::vector<Sub> sub;
  struct Colour {
    long long id = 0;
    int m0 = 0, count = 0;         // members[m0 .. m0 + count)
    bool batched = false;
  };
  std::vector<Colour> colours;
  std::vector<int> members_h, idx_h, rowptr_h, col_h;
  // one resident set of the small members' factors: the plain ones or the (conjugate-)transposed ones of doTranspose
  struct Set {
    DevBuf<int> Lptr, Lcol, Uptr, Ucol, P, Q, Lorder, Uorder, Llvl, Ulvl;
    DevBuf<double> Lval, Uval;
    std::vector<mgk::DdSub> desc_h;
    ~Set() {
      for (DevBuf<int>* d : {&Lptr, &Lcol, &Uptr, &Ucol, &P, &Q, &Lorder, &Uorder, &Llvl, &Ulvl}) d->release();
      Lval.release(); Uval.release();
    }
  };
  Set* fwd = nullptr;
  Set* adj = nullptr;
  DevBuf<mgk::DdSub> desc_fwd, desc_adj;
};

namespace {

void dd_drop_sets(mg_dd* d) {
  delete d->fwd; d->fwd = nullptr;
  delete d->adj; d->adj = nullptr;
  d->desc_fwd.release();
  d->desc_adj.release();
  for (auto& s : d->sub)
    if (s.big) { mg_lu_destroy(s.big); s.big = nullptr; }
  d->finalized = false;
}

int dd_create(bool cx, long long device_id, long long n, const long long* rowptr, const long long* colA, const double* valA,
              long long numSub, const long long* idxptr, const unsigned int* idx, const long long* color, mg_dd** out) {
  const size_t vw = cx ? 2 : 1;
  UploadFence upload_fence;
  if (!out) return fail(MG_ERR_INVALID, "out is null");
  *out = nullptr;
  if (n < 1 || numSub < 1 || !rowptr || !colA || !valA || !idxptr || !idx || !color) return fail(MG_ERR_INVALID, "null or empty argument");
  if (n >= (1LL << 31) - 1 || numSub >= (1LL << 31) - 1) return fail(MG_ERR_UNSUPPORTED, "dimension exceeds int32 device indices");
  if (rowptr[0] != 1) return fail(MG_ERR_INVALID, "rowptr[1] must be 1 (1-based Julia arrays expected)");
  const long long nnz = rowptr[n] - 1;
  if (nnz < 0 || nnz >= (1LL << 31) - 1) return fail(MG_ERR_UNSUPPORTED, "nnz does not fit int32");
  if (idxptr[0] != 1) return fail(MG_ERR_INVALID, "idxptr[1] must be 1 (1-based pointer array expected)");
  for (long long s = 0; s < numSub; ++s)
    if (idxptr[s + 1] <= idxptr[s]) return fail(MG_ERR_INVALID, "sub-domain %lld lists no index (idxptr must increase)", s + 1);
  const long long nidx = idxptr[numSub] - 1;
  if (nidx >= (1LL << 31) - 1) return fail(MG_ERR_UNSUPPORTED, "the index lists hold %lld entries: more than int32 device indices", nidx);
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (ndev <= 0) return fail(MG_ERR_HIP, "no HIP device visible: the Schwarz sweep has no CPU fallback");
  if (device_id < 0 || device_id >= ndev) return fail(MG_ERR_INVALID, "device_id=%lld but %d devices visible", device_id, ndev);
  std::vector<int> rp((size_t)n + 1), ci((size_t)std::max<long long>(nnz, 1)), ix((size_t)nidx);
  for (long long i = 0; i <= n; ++i) {
    const long long v = rowptr[i] - 1;
    if (v < 0 || v > nnz || (i > 0 && v < rp[(size_t)i - 1])) return fail(MG_ERR_INVALID, "rowptr is not a monotone 1-based pointer array");
    rp[(size_t)i] = (int)v;
  }
  for (long long k = 0; k < nnz; ++k) {
    const long long c = colA[k] - 1;
    if (c < 0 || c >= n) return fail(MG_ERR_INVALID, "column index out of range");
    ci[(size_t)k] = (int)c;
  }
  std::vector<long long> seen((size_t)n, -1);   // an index listed twice by one sub-domain would be added to twice
  for (long long s = 0; s < numSub; ++s)
    for (long long t = idxptr[s] - 1; t < idxptr[s + 1] - 1; ++t) {
      const long long g = (long long)idx[t] - 1;
      if (g < 0 || g >= n) return fail(MG_ERR_INVALID, "sub-domain %lld: index %u outside 1..%lld", s + 1, idx[t], n);
      if (seen[(size_t)g] == s) return fail(MG_ERR_INVALID, "sub-domain %lld lists index %u twice", s + 1, idx[t]);
      seen[(size_t)g] = s;
      ix[(size_t)t] = (int)g;
    }
  std::map<long long, std::vector<int>> by_colour;   // ascending colour, linear order inside (DDSerial.jl:116-119)
  for (long long s = 0; s < numSub; ++s) {
    if (color[s] < 1) return fail(MG_ERR_INVALID, "color[%lld]=%lld: colours are 1-based", s + 1, color[s]);
    by_colour[color[s]].push_back((int)s);
  }
  HIP_TRY(hipSetDevice((int)device_id));
  mg_dd* d = new mg_dd();
  d->device = (int)device_id;
  d->cx = cx;
  d->n = n;
  d->nnz = nnz;
  d->numSub = numSub;
  d->multi_min_rows = Options::from_env().lu_multi_min_rows;   // the only place the environment is read for this handle
  d->sub.resize((size_t)numSub);
  for (long long s = 0; s < numSub; ++s) {
    d->sub[(size_t)s].n = idxptr[s + 1] - idxptr[s];
    d->sub[(size_t)s].idx0 = idxptr[s] - 1;
  }
  for (auto& kv : by_colour) {
    mg_dd::Colour c;
    c.id = kv.first;
    c.m0 = (int)d->members_h.size();
    c.count = (int)kv.second.size();
    d->members_h.insert(d->members_h.end(), kv.second.begin(), kv.second.end());
    d->colours.push_back(c);
  }
  auto up = [&]() -> int {
    MG_TRY(d->rowptr.alloc(rp.size()));
    MG_TRY(d->col.alloc(ci.size()));
    MG_TRY(d->val.alloc(vw * (size_t)std::max<long long>(nnz, 1)));
    MG_TRY(d->idx.alloc(ix.size()));
    MG_TRY(d->members.alloc(d->members_h.size()));
    MG_TRY(d->r.alloc(vw * (size_t)nidx));
    MG_TRY(d->y.alloc(vw * (size_t)nidx));
    HIP_TRY(hipMemcpy(d->rowptr.p, rp.data(), rp.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d->col.p, ci.data(), (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d->val.p, valA, vw * (size_t)nnz * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d->idx.p, ix.data(), ix.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d->members.p, d->members_h.data(), d->members_h.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&d->ev_mine, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&d->ev_theirs, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&d->ev_owner, hipEventDisableTiming));
    return MG_OK;
  };
  const int rc = up();
  if (rc != MG_OK) {
    mg_dd_destroy(d);
    return rc;
  }
  d->rowptr_h.swap(rp);   // kept for the independence test of mg_dd_finalize
  d->col_h.swap(ci);
  d->idx_h.swap(ix);
  *out = d;
  return MG_OK;
}

int dd_set_factor(bool cx, mg_dd* d, long long ic, long long n_i, const long long* Lptr, const long long* Lcol, const double* Lval,
                  const long long* Uptr, const long long* Ucol, const double* Uval, const long long* p, const long long* q) {
  if (!d) return fail(MG_ERR_INVALID, "null handle");
  if (d->cx != cx)
    return fail(MG_ERR_STATE, "%s", cx ? "mg_dd_set_factor_CFP64_INT64 on a handle of Float64 values (mg_dd_create_CFP64_INT64)"
                                       : "mg_dd_set_factor_FP64_INT64 on a handle of ComplexF64 values (mg_dd_set_factor_CFP64_INT64)");
  if (ic < 1 || ic > d->numSub) return fail(MG_ERR_INVALID, "sub-domain %lld outside 1..%lld", ic, d->numSub);
  if (n_i < 1 || !Lptr || !Lcol || !Lval || !Uptr || !Ucol || !Uval || !p || !q) return fail(MG_ERR_INVALID, "null or empty factor");
  mg_dd::Sub& S = d->sub[(size_t)ic - 1];
  if (n_i != S.n) return fail(MG_ERR_INVALID, "sub-domain %lld: factors of order %lld, but its index list holds %lld rows", ic, n_i, S.n);
  if (Lptr[0] != 1 || Uptr[0] != 1 || Lptr[n_i] < 1 || Uptr[n_i] < 1) return fail(MG_ERR_INVALID, "row pointers must be 1-based");
  if (Lptr[n_i] - 1 >= (1LL << 31) - 1 || Uptr[n_i] - 1 >= (1LL << 31) - 1) return fail(MG_ERR_UNSUPPORTED, "factors exceed int32 device indices");
  for (long long i = 0; i < n_i; ++i)
    if (Lptr[i + 1] < Lptr[i] || Uptr[i + 1] < Uptr[i]) return fail(MG_ERR_INVALID, "row pointers must not decrease");
  {   // the layout checks of the applier (diagonal positions, triangularity, column range), before anything is kept
    std::vector<int> P, Cc, O, LL;
    MG_TRY(lu_convert(n_i, Lptr, Lcol, true, P, Cc, O, LL));
    MG_TRY(lu_convert(n_i, Uptr, Ucol, false, P, Cc, O, LL));
  }
  for (long long i = 0; i < n_i; ++i)
    if (p[i] < 1 || p[i] > n_i || q[i] < 1 || q[i] > n_i) return fail(MG_ERR_INVALID, "permutation entry out of range");
  (void)hipSetDevice(d->device);
  if (d->stream) (void)spin_sync(d->stream);
  if (d->owner && d->owner->play->stream) (void)spin_sync(d->owner->play->stream);   // (a borrowing hierarchy's sweeps read the sets)
  dd_drop_sets(d);   // (a factor replaced after mg_dd_finalize: finalize again)
  const size_t vw = cx ? 2 : 1;
  const size_t ln = (size_t)(Lptr[n_i] - 1), un = (size_t)(Uptr[n_i] - 1);
  S.Lptr.assign(Lptr, Lptr + n_i + 1);
  S.Uptr.assign(Uptr, Uptr + n_i + 1);
  S.Lcol.assign(Lcol, Lcol + ln);
  S.Ucol.assign(Ucol, Ucol + un);
  S.Lval.assign(Lval, Lval + vw * ln);
  S.Uval.assign(Uval, Uval + vw * un);
  S.p.assign(p, p + n_i);
  S.q.assign(q, q + n_i);
  S.set = true;
  return MG_OK;
}

// Members of one colour are independent when their index sets are pairwise disjoint and no row listed by one stores a
// column listed by another: then no member reads or writes an entry of x that another member writes.
bool dd_colour_independent(const mg_dd* d, const mg_dd::Colour& c, std::vector<int>& owner) {
  bool ok = true;
  for (int m = 0; m < c.count && ok; ++m) {
    const mg_dd::Sub& S = d->sub[(size_t)d->members_h[(size_t)(c.m0 + m)]];
    for (long long t = 0; t < S.n; ++t) {
      int& o = owner[(size_t)d->idx_h[(size_t)(S.idx0 + t)]];
      if (o >= 0 && o != m) { ok = false; break; }
      o = m;
    }
  }
  for (int m = 0; m < c.count && ok; ++m) {
    const mg_dd::Sub& S = d->sub[(size_t)d->members_h[(size_t)(c.m0 + m)]];
    for (long long t = 0; t < S.n && ok; ++t) {
      const int row = d->idx_h[(size_t)(S.idx0 + t)];
      for (int k = d->rowptr_h[(size_t)row]; k < d->rowptr_h[(size_t)row + 1]; ++k) {
        const int o = owner[(size_t)d->col_h[(size_t)k]];
        if (o >= 0 && o != m) { ok = false; break; }
      }
    }
  }
  for (int m = 0; m < c.count; ++m) {   // leave `owner` clean for the next colour
    const mg_dd::Sub& S = d->sub[(size_t)d->members_h[(size_t)(c.m0 + m)]];
    for (long long t = 0; t < S.n; ++t) owner[(size_t)d->idx_h[(size_t)(S.idx0 + t)]] = -1;
  }
  return ok;
}

// The resident set of one solve direction (the small members' factors in shared arenas); the transposed / adjoint set is
// built on its first use and kept beside the plain one, as the applier does (cxlu_set, lu_hierarchy).
int dd_set(mg_dd* d, bool adjoint, mg_dd::Set** out, const mgk::DdSub** desc_dev) {
  mg_dd::Set*& F = adjoint ? d->adj : d->fwd;
  DevBuf<mgk::DdSub>& DD = adjoint ? d->desc_adj : d->desc_fwd;
  if (!F) {
    UploadFence upload_fence;
    std::vector<int> Lptr, Lcol, Uptr, Ucol, P, Q, Lorder, Uorder, Llvl, Ulvl;
    std::vector<double> Lval, Uval;
    std::vector<mgk::DdSub> desc((size_t)d->numSub);
    std::vector<long long> lp, lc, up, uc;
    std::vector<double> lv, uv;
    std::vector<int> LP, LC, LO, LL, UP, UC, UO, UL;
    for (long long s = 0; s < d->numSub; ++s) {
      const mg_dd::Sub& S = d->sub[(size_t)s];
      mgk::DdSub& e = desc[(size_t)s];
      e = mgk::DdSub{};
      e.n = (int)S.n;
      e.vec0 = (int)S.idx0;
      if (S.big) continue;   // (its own applier holds its factors)
      const std::vector<long long>*pl = &S.Lptr, *cl = &S.Lcol, *pu = &S.Uptr, *cu = &S.Ucol, *pp = &S.p, *qq = &S.q;
      const std::vector<double>*vl = &S.Lval, *vu = &S.Uval;
      if (adjoint) {   // x[p] = L' \ (U' \ b[q]) (parLU.cpp:194-260; ' conjugates for complex values): U' takes L's place
        if (d->cx) {
          cx_adjoint_csr1(S.n, S.Uptr, S.Ucol, S.Uval, lp, lc, lv);
          cx_adjoint_csr1(S.n, S.Lptr, S.Lcol, S.Lval, up, uc, uv);
        } else {
          transpose_csr1(S.n, S.Uptr, S.Ucol, S.Uval, lp, lc, lv);
          transpose_csr1(S.n, S.Lptr, S.Lcol, S.Lval, up, uc, uv);
        }
        pl = &lp; cl = &lc; vl = &lv; pu = &up; cu = &uc; vu = &uv; pp = &S.q; qq = &S.p;
      }
      MG_TRY(lu_convert(S.n, pl->data(), cl->data(), true, LP, LC, LO, LL));
      MG_TRY(lu_convert(S.n, pu->data(), cu->data(), false, UP, UC, UO, UL));
      if (Lptr.size() + LP.size() >= (1ULL << 31) || Lcol.size() + LC.size() >= (1ULL << 31) || Ucol.size() + UC.size() >= (1ULL << 31) ||
          Llvl.size() + LL.size() >= (1ULL << 31) || Ulvl.size() + UL.size() >= (1ULL << 31))
        return fail(MG_ERR_UNSUPPORTED, "the packed factors exceed int32 device indices");
      e.ptr0 = (int)Lptr.size();
      e.Lnz0 = (int)Lcol.size();
      e.Unz0 = (int)Ucol.size();
      e.Llvl0 = (int)Llvl.size(); e.nLlvl = (int)LL.size() - 1;
      e.Ulvl0 = (int)Ulvl.size(); e.nUlvl = (int)UL.size() - 1;
      Lptr.insert(Lptr.end(), LP.begin(), LP.end());
      Uptr.insert(Uptr.end(), UP.begin(), UP.end());
      Lcol.insert(Lcol.end(), LC.begin(), LC.end());
      Ucol.insert(Ucol.end(), UC.begin(), UC.end());
      Lval.insert(Lval.end(), vl->begin(), vl->end());
      Uval.insert(Uval.end(), vu->begin(), vu->end());
      Llvl.insert(Llvl.end(), LL.begin(), LL.end());
      Ulvl.insert(Ulvl.end(), UL.begin(), UL.end());
      // p, q, Lorder, Uorder sit at the sub-domain's place in the index arena (vec0): pad up to it
      P.resize((size_t)S.idx0, 0); Q.resize((size_t)S.idx0, 0); Lorder.resize((size_t)S.idx0, 0); Uorder.resize((size_t)S.idx0, 0);
      for (long long i = 0; i < S.n; ++i) {
        P.push_back((int)((*pp)[(size_t)i] - 1));
        Q.push_back((int)((*qq)[(size_t)i] - 1));
      }
      Lorder.insert(Lorder.end(), LO.begin(), LO.end());
      Uorder.insert(Uorder.end(), UO.begin(), UO.end());
    }
    mg_dd::Set* G = new mg_dd::Set();
    auto up_i = [&](DevBuf<int>& b, const std::vector<int>& v) -> int {
      MG_TRY(b.alloc(v.size()));
      if (!v.empty()) HIP_TRY(hipMemcpy(b.p, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
      return MG_OK;
    };
    auto up_d = [&](DevBuf<double>& b, const std::vector<double>& v) -> int {
      MG_TRY(b.alloc(v.size()));
      if (!v.empty()) HIP_TRY(hipMemcpy(b.p, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
      return MG_OK;
    };
    auto upload = [&]() -> int {
      MG_TRY(up_i(G->Lptr, Lptr)); MG_TRY(up_i(G->Lcol, Lcol)); MG_TRY(up_i(G->Uptr, Uptr)); MG_TRY(up_i(G->Ucol, Ucol));
      MG_TRY(up_i(G->P, P)); MG_TRY(up_i(G->Q, Q)); MG_TRY(up_i(G->Lorder, Lorder)); MG_TRY(up_i(G->Uorder, Uorder));
      MG_TRY(up_i(G->Llvl, Llvl)); MG_TRY(up_i(G->Ulvl, Ulvl));
      MG_TRY(up_d(G->Lval, Lval)); MG_TRY(up_d(G->Uval, Uval));
      MG_TRY(DD.alloc(desc.size()));
      HIP_TRY(hipMemcpy(DD.p, desc.data(), desc.size() * sizeof(mgk::DdSub), hipMemcpyHostToDevice));
      return MG_OK;
    };
    const int rc = upload();
    if (rc != MG_OK) {
      delete G;
      return rc;
    }
    G->desc_h.swap(desc);
    F = G;
  }
  *out = F;
  *desc_dev = DD.p;
  return MG_OK;
}

// niter sweeps enqueued on `stream` (the handle's own, or the stream a borrowing hierarchy plays on).  from_zero: x is zero-filled
// on the stream first, so the caller's x is never read.  (A first colour that takes r = b[I] instead of (b - A x)[I] was measured
// and is not faster: profiles/coarse_solver.md, the variant in profiles/coarse_solver_from_zero_variant.patch.)
template <typename T>
int dd_sweeps(mg_dd* d, hipStream_t stream, mg_dd::Set& G, const mgk::DdSub* desc_dev, const T* b, T* x, long long niter, bool adjoint,
              bool from_zero) {
  mgk::DdDevT<T> D;
  D.rowptr = d->rowptr.p; D.col = d->col.p; D.val = reinterpret_cast<const T*>(d->val.p);
  D.idx = d->idx.p; D.sub = desc_dev; D.members = d->members.p;
  D.Lptr = G.Lptr.p; D.Lcol = G.Lcol.p; D.Lval = reinterpret_cast<const T*>(G.Lval.p); D.Lorder = G.Lorder.p; D.Llvl = G.Llvl.p;
  D.Uptr = G.Uptr.p; D.Ucol = G.Ucol.p; D.Uval = reinterpret_cast<const T*>(G.Uval.p); D.Uorder = G.Uorder.p; D.Ulvl = G.Ulvl.p;
  D.p = G.P.p; D.q = G.Q.p;
  D.r = reinterpret_cast<T*>(d->r.p); D.y = reinterpret_cast<T*>(d->y.p);
  T* w = reinterpret_cast<T*>(d->w.p);
  if (from_zero) HIP_TRY(hipMemsetAsync(x, 0, (size_t)d->n * sizeof(T), stream));
  for (long long it = 0; it < niter; ++it)
    for (const mg_dd::Colour& c : d->colours) {
      if (c.batched) {
        hipLaunchKernelGGL(mgk::dd_color_sweep<T>, dim3((unsigned)c.count), dim3(1024), 0, stream, D, c.m0, b, x);
        continue;
      }
      for (int m = 0; m < c.count; ++m) {
        const int s = d->members_h[(size_t)(c.m0 + m)];
        const mg_dd::Sub& S = d->sub[(size_t)s];
        const mgk::DdSub& e = G.desc_h[(size_t)s];
        const int n_i = e.n;
        const int* I = d->idx.p + e.vec0;
        T* r = D.r + e.vec0;
        T* t = D.y + e.vec0;
        hipLaunchKernelGGL(mgk::dd_gather_residual<T>, dim3((unsigned)(((long long)n_i * 8 + mgk::BLK - 1) / mgk::BLK)), dim3(mgk::BLK), 0,
                           stream, D.rowptr, D.col, D.val, I, n_i, b, x, r);
        if (!S.big) {
          mgk::LuDevT<T> F;
          F.n = n_i;
          F.Lptr = D.Lptr + e.ptr0; F.Lcol = D.Lcol + e.Lnz0; F.Lval = D.Lval + e.Lnz0;
          F.Uptr = D.Uptr + e.ptr0; F.Ucol = D.Ucol + e.Unz0; F.Uval = D.Uval + e.Unz0;
          F.p = D.p + e.vec0; F.q = D.q + e.vec0;
          F.Lorder = D.Lorder + e.vec0; F.Llvl = D.Llvl + e.Llvl0; F.nLlvl = e.nLlvl;
          F.Uorder = D.Uorder + e.vec0; F.Ulvl = D.Ulvl + e.Ulvl0; F.nUlvl = e.nUlvl;
          hipLaunchKernelGGL(mgk::sptrsv_lu<T>, dim3(1), dim3(1024), 0, stream, F, r, t, w, 1);
        } else {
          // the member's own applier enqueues on a stream of its own: order it behind the gather, and the scatter behind it
          hipStream_t theirs;
          HIP_TRY(hipEventRecord(d->ev_mine, stream));
          if (S.big->cx) {
            CxLuSet* LS = nullptr;
            MG_TRY(cxlu_set(S.big->cx, adjoint, &LS));
            theirs = S.big->cx->stream;
            HIP_TRY(hipStreamWaitEvent(theirs, d->ev_mine, 0));
            MG_TRY(cxlu_solve_dev(S.big->cx, *LS, reinterpret_cast<const cx_t*>(r), reinterpret_cast<cx_t*>(t), 1));
          } else {
            mg_hierarchy* h = nullptr;
            MG_TRY(lu_hierarchy(S.big, adjoint, &h));
            MG_TRY(check_ready(h, n_i, 1));   // (created for one right-hand side and private to this handle: nrhs stays 1)
            theirs = h->play->stream;
            HIP_TRY(hipStreamWaitEvent(theirs, d->ev_mine, 0));
            MG_TRY(cycle_dev(h, reinterpret_cast<const double*>(r), reinterpret_cast<double*>(t), true));
          }
          HIP_TRY(hipEventRecord(d->ev_theirs, theirs));
          HIP_TRY(hipStreamWaitEvent(stream, d->ev_theirs, 0));
        }
        hipLaunchKernelGGL(mgk::dd_scatter_add<T>, dim3((unsigned)((n_i + mgk::BLK - 1) / mgk::BLK)), dim3(mgk::BLK), 0, stream, I,
                           n_i, t, x);
      }
    }
  HIP_TRY(hipGetLastError());
  return MG_OK;
}

// The arguments of an apply and the handle's value type (cx: the entry point's)
int dd_args(bool cx, mg_dd* d, const double* b, const double* x, long long n, long long niter, const char* name) {
  if (!d) return fail(MG_ERR_INVALID, "null handle");
  if (d->cx != cx)
    return fail(MG_ERR_STATE, "%s on a handle of %s values (%s)", name, d->cx ? "ComplexF64" : "Float64",
                d->cx ? "mg_dd_apply*_CFP64" : "mg_dd_apply*_FP64");
  if (!d->finalized) return fail(MG_ERR_STATE, "%s before mg_dd_finalize", name);
  if (n != d->n) return fail(MG_ERR_INVALID, "n=%lld but the operator has order %lld", n, d->n);
  if (!b || !x || b == x || niter < 0) return fail(MG_ERR_INVALID, "bad argument (b and x must be two vectors)");
  (void)hipSetDevice(d->device);
  return MG_OK;
}

// niter sweeps on device vectors, enqueued on `stream` (no synchronisation); from_zero: from x = 0, whatever x holds
int dd_run(mg_dd* d, hipStream_t stream, const double* b_dev, double* x_dev, long long niter, long long doTranspose, bool from_zero = false) {
  mg_dd::Set* G = nullptr;
  const mgk::DdSub* desc_dev = nullptr;
  MG_TRY(dd_set(d, doTranspose != 0, &G, &desc_dev));
  if (d->cx)
    return dd_sweeps<cx_t>(d, stream, *G, desc_dev, reinterpret_cast<const cx_t*>(b_dev), reinterpret_cast<cx_t*>(x_dev), niter,
                           doTranspose != 0, from_zero);
  return dd_sweeps<double>(d, stream, *G, desc_dev, b_dev, x_dev, niter, doTranspose != 0, from_zero);
}

// A stand-alone sweep on a handle that a hierarchy borrows shares the handle's scratch with that hierarchy's cycles: the
// handle's stream waits for what the hierarchy has enqueued so far (the stand-alone entry points synchronise before they return,
// so the hierarchy's next cycle is behind them)
int dd_behind_owner(mg_dd* d) {
  if (!d->owner) return MG_OK;
  HIP_TRY(hipEventRecord(d->ev_owner, d->owner->play->stream));
  HIP_TRY(hipStreamWaitEvent(d->stream, d->ev_owner, 0));
  return MG_OK;
}

// the coarsest solve of a hierarchy (k_coarse / cx_coarse): one sweep with doTranspose = 0 on the stream being played - from
// zero, or (one level only, MGcycle.jl:13-18) from the caller's x
int dd_coarse(mg_hierarchy* h, const double* b, double* x, bool x_zero) {
  if (!h->coarse_dd->finalized) return fail(MG_ERR_STATE, "the sweep handle of the coarsest solve is not finalized (mg_dd_finalize)");
  return dd_run(h->coarse_dd, h->play->stream, b, x, 1, 0, x_zero);
}
void dd_detach(mg_hierarchy* h) {
  if (!h->coarse_dd) return;
  h->coarse_dd->owner = nullptr;
  h->coarse_dd = nullptr;
}

int dd_apply_dev(bool cx, mg_dd* d, const double* b_dev, double* x_dev, long long n, long long niter, long long doTranspose,
                 const char* name, bool from_zero = false) {
  MG_TRY(dd_args(cx, d, b_dev, x_dev, n, niter, name));
  MG_TRY(dd_behind_owner(d));
  MG_TRY(dd_run(d, d->stream, b_dev, x_dev, niter, doTranspose, from_zero));
  HIP_TRY(spin_sync(d->stream));
  return MG_OK;
}

int dd_apply_host(bool cx, mg_dd* d, const double* b, double* x, long long n, long long niter, long long doTranspose, const char* name,
                  bool from_zero = false) {
  MG_TRY(dd_args(cx, d, b, x, n, niter, name));
  const size_t len = (cx ? 2 : 1) * (size_t)n;   // doubles
  if (d->stage_b.n != len) {
    MG_TRY(d->stage_b.alloc(len));
    MG_TRY(d->stage_x.alloc(len));
  }
  MG_TRY(dd_behind_owner(d));
  HIP_TRY(hipMemcpyAsync(d->stage_b.p, b, len * sizeof(double), hipMemcpyHostToDevice, d->stream));
  if (!from_zero) HIP_TRY(hipMemcpyAsync(d->stage_x.p, x, len * sizeof(double), hipMemcpyHostToDevice, d->stream));
  MG_TRY(dd_run(d, d->stream, d->stage_b.p, d->stage_x.p, niter, doTranspose, from_zero));
  HIP_TRY(hipMemcpyAsync(x, d->stage_x.p, len * sizeof(double), hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(spin_sync(d->stream));
  return MG_OK;
}

}  // namespace

extern "C" {

// rowptr / colA / valA: CSR of the applied operator A (1-based Int64) - the reference's AT.colptr / AT.rowval and
// conj(AT.nzval) (computeResidualAtIdx, DDSerial.jl:4-20).  idx: the index lists GlobalIndices[ic] (DDIndType = UInt32,
// 1-based, DomainDecomposition.jl:15) back to back, sub-domain ic at idxptr[ic] .. idxptr[ic+1]-1 (1-based); color[ic]
// its colour (cellColor, Vanka.jl:105-130).
int mg_dd_create_FP64_INT64(long long device_id, long long n, const long long* rowptr, const long long* colA, const double* valA,
                            long long numSub, const long long* idxptr, const unsigned int* idx, const long long* color, mg_dd** out) {
  return dd_create(false, device_id, n, rowptr, colA, valA, numSub, idxptr, idx, color, out);
}
int mg_dd_create_CFP64_INT64(long long device_id, long long n, const long long* rowptr, const long long* colA, const double* valA,
                             long long numSub, const long long* idxptr, const unsigned int* idx, const long long* color, mg_dd** out) {
  return dd_create(true, device_id, n, rowptr, colA, valA, numSub, idxptr, idx, color, out);
}

int mg_dd_set_factor_FP64_INT64(mg_dd* dd, long long ic, long long n_i, const long long* Lptr, const long long* Lcol, const double* Lval,
                                const long long* Uptr, const long long* Ucol, const double* Uval, const long long* p, const long long* q) {
  return dd_set_factor(false, dd, ic, n_i, Lptr, Lcol, Lval, Uptr, Ucol, Uval, p, q);
}
int mg_dd_set_factor_CFP64_INT64(mg_dd* dd, long long ic, long long n_i, const long long* Lptr, const long long* Lcol, const double* Lval,
                                 const long long* Uptr, const long long* Ucol, const double* Uval, const long long* p, const long long* q) {
  return dd_set_factor(true, dd, ic, n_i, Lptr, Lcol, Lval, Uptr, Ucol, Uval, p, q);
}

int mg_dd_finalize(mg_dd* d) {
  if (!d) return fail(MG_ERR_INVALID, "null handle");
  for (long long s = 0; s < d->numSub; ++s)
    if (!d->sub[(size_t)s].set) return fail(MG_ERR_STATE, "sub-domain %lld has no factors (mg_dd_set_factor_*)", s + 1);
  (void)hipSetDevice(d->device);
  if (d->stream) (void)spin_sync(d->stream);
  if (d->owner && d->owner->play->stream) (void)spin_sync(d->owner->play->stream);
  dd_drop_sets(d);
  long long wmax = 0;
  std::vector<int> owner((size_t)d->n, -1);
  for (mg_dd::Colour& c : d->colours) {
    bool large = false;
    for (int m = 0; m < c.count; ++m) large = large || d->sub[(size_t)d->members_h[(size_t)(c.m0 + m)]].n >= d->multi_min_rows;
    c.batched = !large && dd_colour_independent(d, c, owner);
    if (c.batched) continue;
    for (int m = 0; m < c.count; ++m) {
      mg_dd::Sub& S = d->sub[(size_t)d->members_h[(size_t)(c.m0 + m)]];
      if (S.n < d->multi_min_rows) {
        wmax = std::max(wmax, S.n);
        continue;
      }
      // a large member: the applier's own handle (it selects the chip-wide form by the same option)
      MG_TRY((d->cx ? mg_lu_create_CFP64_INT64 : mg_lu_create_FP64_INT64)(d->device, S.n, S.Lptr.data(), S.Lcol.data(), S.Lval.data(),
                                                                          S.Uptr.data(), S.Ucol.data(), S.Uval.data(), S.p.data(),
                                                                          S.q.data(), &S.big));
      long long f[7];
      MG_TRY(mg_lu_form(S.big, 0, f));
      S.big_launches = f[1] ? f[3] + f[4] + (f[2] > 0 ? 3 : 0) + 1 : 1;   // levels, the trailing block's three kernels, the scatter
    }
  }
  if (wmax > 0) MG_TRY(d->w.alloc((d->cx ? 2 : 1) * (size_t)wmax));
  mg_dd::Set* G = nullptr;
  const mgk::DdSub* desc_dev = nullptr;
  MG_TRY(dd_set(d, false, &G, &desc_dev));
  d->finalized = true;
  return MG_OK;
}

// b, x: host vectors of n values (x in/out); niter sweeps; doTranspose reaches the sub-domain solves only (DDSerial.jl:128)
int mg_dd_apply_FP64(mg_dd* d, const double* b, double* x, long long n, long long niter, long long doTranspose) {
  return dd_apply_host(false, d, b, x, n, niter, doTranspose, "mg_dd_apply_FP64");
}
int mg_dd_apply_CFP64(mg_dd* d, const double* b, double* x, long long n, long long niter, long long doTranspose) {
  return dd_apply_host(true, d, b, x, n, niter, doTranspose, "mg_dd_apply_CFP64");
}
int mg_dd_apply_dev_FP64(mg_dd* d, const double* b_dev, double* x_dev, long long n, long long niter, long long doTranspose) {
  return dd_apply_dev(false, d, b_dev, x_dev, n, niter, doTranspose, "mg_dd_apply_dev_FP64");
}
int mg_dd_apply_dev_CFP64(mg_dd* d, const double* b_dev, double* x_dev, long long n, long long niter, long long doTranspose) {
  return dd_apply_dev(true, d, b_dev, x_dev, n, niter, doTranspose, "mg_dd_apply_dev_CFP64");
}

// One sweep from x = 0 (what getDDpreconditioner and the cycle's coarsest solve ask for): x is output only - it is zero-filled on
// the stream, then swept.
int mg_dd0_apply_FP64(mg_dd* d, const double* b, double* x, long long n, long long doTranspose) {
  return dd_apply_host(false, d, b, x, n, 1, doTranspose, "mg_dd0_apply_FP64", true);
}
int mg_dd0_apply_CFP64(mg_dd* d, const double* b, double* x, long long n, long long doTranspose) {
  return dd_apply_host(true, d, b, x, n, 1, doTranspose, "mg_dd0_apply_CFP64", true);
}
int mg_dd0_apply_dev_FP64(mg_dd* d, const double* b_dev, double* x_dev, long long n, long long doTranspose) {
  return dd_apply_dev(false, d, b_dev, x_dev, n, 1, doTranspose, "mg_dd0_apply_dev_FP64", true);
}
int mg_dd0_apply_dev_CFP64(mg_dd* d, const double* b_dev, double* x_dev, long long n, long long doTranspose) {
  return dd_apply_dev(true, d, b_dev, x_dev, n, 1, doTranspose, "mg_dd0_apply_dev_CFP64", true);
}

// The coarsest solve of a hierarchy by one sweep of a finalized handle (MGsetup.jl:323-326, MGcycle.jl:140-143).  The hierarchy
// borrows the handle; dd == NULL detaches it and leaves the coarsest solve unset.
int mg_set_coarse_dd(mg_hierarchy* h, mg_dd* d) {
  if (!h) return fail(MG_ERR_INVALID, "null hierarchy handle");
  (void)hipSetDevice(h->device);
  graphs_clear(h);
  if (h->play->stream) HIP_TRY(spin_sync(h->play->stream));
  if (!d) {
    const bool was = h->coarse_dd != nullptr;
    dd_detach(h);
    if (was) {
      if (h->cx) { h->cx->coarse_set = false; h->cx->finalized = false; }
      else { h->coarse_set = false; h->finalized = false; }
    }
    return MG_OK;
  }
  if (d->cx != (h->cx != nullptr))
    return fail(MG_ERR_STATE, "mg_set_coarse_dd: a sweep handle of %s values on a hierarchy of %s values", d->cx ? "ComplexF64" : "Float64",
                h->cx ? "ComplexF64" : "Float64");
  if (h->cx && h->cx->single) return fail(MG_ERR_UNSUPPORTED, "a Schwarz sweep as coarsest solve is not served for CF32 handles");
  if (!d->finalized) return fail(MG_ERR_STATE, "mg_set_coarse_dd before mg_dd_finalize");
  if (d->owner && d->owner != h) return fail(MG_ERR_STATE, "the sweep handle is the coarsest solve of another hierarchy");
  if (d->device != h->device) return fail(MG_ERR_INVALID, "the sweep handle lives on device %d, the hierarchy on device %d", d->device, h->device);
  if (h->ghost) return fail(MG_ERR_UNSUPPORTED, "a Schwarz sweep as coarsest solve is not served on sharded hierarchies");
  if (h->lu_only) return fail(MG_ERR_INVALID, "a factor applier's handle has no coarsest solve to replace");
  dd_detach(h);
  h->coarse_dd = d;
  d->owner = h;
  if (h->cx) {
    CxState& S = *h->cx;
    cx_drop_coarse_appliers(S);
    S.n_coarse = d->n;
    S.coarse_set = true;
    S.coarse_lu = false;
    S.coarse_gmres = false;
    S.Ainv.release();
    S.finalized = false;
  } else {
    h->n_coarse = d->n;
    h->coarse_set = true;
    h->coarse_lu = false;
    h->coarse_gmres = false;
    h->Ainv.release();
    h->finalized = false;
  }
  return MG_OK;
}

// info[0]: the coarsest solve in use - 0 dense inverse, 1 sparse LU in one workgroup, 2 sparse LU chip-wide, 3 GMRES, 4 Schwarz
// sweep; info[1]: its order; info[2]: kernel launches per solve (GMRES on a real handle: 0, it depends on the right-hand side; on a
// complex handle the whole speculative solve, which does not: front, 10 steps, combination - on the path the handle takes now)
int mg_coarse_form(mg_hierarchy* h, long long* info) {
  if (!h || !info) return fail(MG_ERR_INVALID, "null argument");
  const bool set = h->cx ? h->cx->coarse_set : h->coarse_set;
  if (!set) return fail(MG_ERR_STATE, "the coarsest solve was not set");
  info[1] = h->cx ? h->cx->n_coarse : h->n_coarse;
  if (h->coarse_dd) {
    long long f[6];
    MG_TRY(mg_dd_info(h->coarse_dd, f));
    info[0] = 4;
    info[2] = f[5];
  } else if (h->cx) {
    const CxState& S = *h->cx;
    info[0] = S.coarse_gmres ? 3 : S.coarse_multi ? 2 : S.coarse_lu ? 1 : 0;
    info[2] = S.coarse_gmres ? cx_cg_launches(h) : 1;
    if (S.coarse_multi) {
      const CxLuSet& G = *S.coarse_multi->fwd;
      info[2] = G.multi ? (long long)(G.Llvl_h.size() - 1) + (long long)(G.Ulvl_h.size() - 1) + (G.M > 0 ? 3 : 0) + 1 : 1;
    } else if (S.coarse_single) {   // ComplexF32 factors: one applier holds either form
      const CxLuSetT<cf_t>& G = *S.coarse_single->fwd;
      if (G.multi) {
        info[0] = 2;
        info[2] = (long long)(G.Llvl_h.size() - 1) + (long long)(G.Ulvl_h.size() - 1) + (G.M > 0 ? 3 : 0) + 1;
      }
    }
  } else if (h->coarse_gmres) {
    info[0] = 3;
    info[2] = 0;
  } else if (h->coarse_lu) {
    info[0] = h->lu_multi ? 2 : 1;
    info[2] = h->lu_multi ? (long long)(h->luLlvl_h.size() - 1) + (long long)(h->luUlvl_h.size() - 1) + (h->luML > 0 ? 2 : 0) + (h->luMU > 0 ? 1 : 0) + 1 : 1;
  } else {
    info[0] = 0;
    info[2] = 1;
  }
  return MG_OK;
}

// info[0..6): value type (0 Float64, 1 ComplexF64); sub-domains; colours present; colours run batched; colours run in
// sequence; kernel launches of one sweep (doTranspose = 0; a chip-wide member counts its levels)
int mg_dd_info(mg_dd* d, long long* info) {
  if (!d || !info) return fail(MG_ERR_INVALID, "null argument");
  if (!d->finalized) return fail(MG_ERR_STATE, "mg_dd_info before mg_dd_finalize");
  long long batched = 0, launches = 0;
  for (const mg_dd::Colour& c : d->colours) {
    if (c.batched) {
      ++batched;
      ++launches;
      continue;
    }
    for (int m = 0; m < c.count; ++m) {
      const mg_dd::Sub& S = d->sub[(size_t)d->members_h[(size_t)(c.m0 + m)]];
      launches += 2 + (S.big ? S.big_launches : 1);
    }
  }
  info[0] = d->cx ? 1 : 0;
  info[1] = d->numSub;
  info[2] = (long long)d->colours.size();
  info[3] = batched;
  info[4] = (long long)d->colours.size() - batched;
  info[5] = launches;
  return MG_OK;
}

// Measurement: device time of one sweep on device vectors, as mg_lu_time_dev measures a solve - `warmup` untimed sweeps,
// then `reps` sweeps, each between two events on the handle's stream; ms[0..reps) in milliseconds.  x is swept in place.
int mg_dd_time_dev(mg_dd* d, const double* b_dev, double* x_dev, long long n, long long doTranspose, long long warmup, long long reps,
                   double* ms) {
  if (!d || !ms || reps < 1 || warmup < 0) return fail(MG_ERR_INVALID, "bad argument");
  MG_TRY(dd_args(d->cx, d, b_dev, x_dev, n, 0, "mg_dd_time_dev"));
  MG_TRY(dd_behind_owner(d));
  MG_TRY(dd_run(d, d->stream, b_dev, x_dev, 0, doTranspose));   // the direction's set is built before the first sample
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = MG_OK;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) rc = fail(MG_ERR_HIP, "hipEventCreate failed");
  for (long long it = 0; it < warmup + reps && rc == MG_OK; ++it) {
    if (hipEventRecord(e0, d->stream) != hipSuccess) rc = fail(MG_ERR_HIP, "hipEventRecord failed");
    if (rc == MG_OK) rc = dd_run(d, d->stream, b_dev, x_dev, 1, doTranspose);
    if (rc == MG_OK) {
      float t = 0.f;
      if (hipEventRecord(e1, d->stream) != hipSuccess || spin_sync(d->stream) != hipSuccess || hipEventElapsedTime(&t, e0, e1) != hipSuccess)
        rc = fail(MG_ERR_HIP, "event timing failed");
      if (it >= warmup) ms[it - warmup] = (double)t;
    }
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  return rc;
}

int mg_dd_destroy(mg_dd* d) {
  if (!d) return MG_OK;
  if (d->owner) return fail(MG_ERR_STATE, "the sweep handle is the coarsest solve of a hierarchy: detach it first (mg_set_coarse_dd(h, NULL) or mg_destroy)");
  (void)hipSetDevice(d->device);
  if (d->stream) (void)spin_sync(d->stream);
  dd_drop_sets(d);
  if (d->ev_mine) (void)hipEventDestroy(d->ev_mine);
  if (d->ev_theirs) (void)hipEventDestroy(d->ev_theirs);
  if (d->ev_owner) (void)hipEventDestroy(d->ev_owner);
  if (d->stream) (void)hipStreamDestroy(d->stream);
  for (DevBuf<int>* b : {&d->rowptr, &d->col, &d->idx, &d->members}) b->release();
  for (DevBuf<double>* b : {&d->val, &d->r, &d->y, &d->w, &d->stage_b, &d->stage_x}) b->release();
  delete d;
  return MG_OK;
}

}  // extern "C"
