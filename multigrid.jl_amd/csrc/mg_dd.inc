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
//
// Value types.  A handle is of one kind, the factor applier's codes: 0 Float64, 1 ComplexF64, 2 Float32, 3 ComplexF32.  Everything
// that holds values - the operator, the caller's factors, the packed arenas, the work and staging vectors - lives in DdVals<V>, V the
// stored type of the kernels (double, cx_t, float, cf_t); the code below is written once over V (dd_store<V>: the host scalar and
// how many make one value).  A single handle keeps all of it in float: no double copy stands beside it.
template <typename V> struct dd_store;
template <> struct dd_store<double> { typedef double scalar; static constexpr int comps = 1; static constexpr int kind = 0; };
template <> struct dd_store<cx_t> { typedef double scalar; static constexpr int comps = 2; static constexpr int kind = 1; };
template <> struct dd_store<float> { typedef float scalar; static constexpr int comps = 1; static constexpr int kind = 2; };
template <> struct dd_store<cf_t> { typedef float scalar; static constexpr int comps = 2; static constexpr int kind = 3; };
template <typename V>
struct DdVals {
  typedef V value;
  typedef typename dd_store<V>::scalar scalar;
  DevBuf<V> val, r, y, w, stage_b, stage_x;
  std::vector<std::vector<scalar>> Lval, Uval;   // the caller's factor values, one pair per sub-domain
  // one resident set of the small members' factors: the plain ones or the (conjugate-)transposed ones of doTranspose
  struct Set {
    DevBuf<int> Lptr, Lcol, Uptr, Ucol, P, Q, Lorder, Uorder, Llvl, Ulvl;
    DevBuf<V> Lval, Uval;
    std::vector<mgk::DdSub> desc_h;
    ~Set() {
      for (DevBuf<int>* d : {&Lptr, &Lcol, &Uptr, &Ucol, &P, &Q, &Lorder, &Uorder, &Llvl, &Ulvl}) d->release();
      Lval.release(); Uval.release();
    }
  };
  Set* fwd = nullptr;
  Set* adj = nullptr;
  void drop_sets() {
    delete fwd; fwd = nullptr;
    delete adj; adj = nullptr;
  }
  ~DdVals() {
    drop_sets();
    for (DevBuf<V>* b : {&val, &r, &y, &w, &stage_b, &stage_x}) b->release();
  }
};
struct mg_dd {
  int device = 0;
  int kind = 0;                    // value type: 0 Float64, 1 ComplexF64, 2 Float32, 3 ComplexF32; the matching member below is set
  DdVals<double>* vd = nullptr;
  DdVals<cx_t>* vz = nullptr;
  DdVals<float>* vs = nullptr;
  DdVals<cf_t>* vc = nullptr;
  long long n = 0, nnz = 0, numSub = 0;
  long long multi_min_rows = 0;    // lu_multi_min_rows, read once at create
  bool finalized = false;
  hipStream_t stream = nullptr;
  hipEvent_t ev_mine = nullptr, ev_theirs = nullptr;   // ordering against the stream of a member's own applier
  mg_hierarchy* owner = nullptr;   // mg_set_coarse_dd: the hierarchy that borrows this handle as its coarsest solve
  hipEvent_t ev_owner = nullptr;   // ... and the event that orders a stand-alone sweep behind that hierarchy's enqueued work
  DevBuf<int> rowptr, col, idx, members;
  struct Sub {
    long long n = 0, idx0 = 0;
    bool set = false;
    std::vector<long long> Lptr, Lcol, Uptr, Ucol, p, q;   // the caller's factors (1-based): the adjoint set is derived from them
    mg_lu* big = nullptr;         // a member of >= multi_min_rows rows: an applier of its own (chip-wide form)
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
  DevBuf<mgk::DdSub> desc_fwd, desc_adj;
};

namespace {

template <typename V> DdVals<V>*& dd_vals(mg_dd* d);
template <> DdVals<double>*& dd_vals<double>(mg_dd* d) { return d->vd; }
template <> DdVals<cx_t>*& dd_vals<cx_t>(mg_dd* d) { return d->vz; }
template <> DdVals<float>*& dd_vals<float>(mg_dd* d) { return d->vs; }
template <> DdVals<cf_t>*& dd_vals<cf_t>(mg_dd* d) { return d->vc; }
// the four kinds behind one call: fn(W) with W the handle's DdVals<V>*
template <typename FN>
auto dd_with(mg_dd* d, FN&& fn) {
  return d->kind == 0 ? fn(d->vd) : d->kind == 1 ? fn(d->vz) : d->kind == 2 ? fn(d->vs) : fn(d->vc);
}
// the suffix of the entry points that serve a kind
const char* dd_kind_sfx(int kind) { return kind == 0 ? "FP64" : kind == 1 ? "CFP64" : kind == 2 ? "FP32" : "CFP32"; }

void dd_drop_sets(mg_dd* d) {
  dd_with(d, [](auto* W) { if (W) W->drop_sets(); return 0; });
  d->desc_fwd.release();
  d->desc_adj.release();
  for (auto& s : d->sub)
    if (s.big) { mg_lu_destroy(s.big); s.big = nullptr; }
  d->finalized = false;
}

template <typename V>
int dd_create(long long device_id, long long n, const long long* rowptr, const long long* colA, const typename dd_store<V>::scalar* valA,
              long long numSub, const long long* idxptr, const unsigned int* idx, const long long* color, mg_dd** out) {
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
  d->kind = dd_store<V>::kind;
  DdVals<V>* W = dd_vals<V>(d) = new DdVals<V>();
  W->Lval.resize((size_t)numSub);
  W->Uval.resize((size_t)numSub);
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
    MG_TRY(W->val.alloc((size_t)std::max<long long>(nnz, 1)));
    MG_TRY(d->idx.alloc(ix.size()));
    MG_TRY(d->members.alloc(d->members_h.size()));
    MG_TRY(W->r.alloc((size_t)nidx));
    MG_TRY(W->y.alloc((size_t)nidx));
    HIP_TRY(hipMemcpy(d->rowptr.p, rp.data(), rp.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d->col.p, ci.data(), (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(W->val.p, valA, (size_t)nnz * sizeof(V), hipMemcpyHostToDevice));
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

// the set-factor entry points that serve a handle's kind
const char* dd_factor_names(int kind) {
  return kind == 0 ? "mg_dd_set_factor_FP64_INT64" : kind == 1 ? "mg_dd_set_factor_CFP64_INT64" : kind == 2 ? "mg_dd_set_factor_FP32_UINT32"
                                                                                               : "mg_dd_set_factor_CFP32_UINT32 / _INT64";
}
// IDX: the index type the caller's column indices and permutations come in (Int64, or the UInt32 of two single forms: widened here)
template <typename V, typename IDX>
int dd_set_factor(mg_dd* d, long long ic, long long n_i, const long long* Lptr, const IDX* Lcol_in, const typename dd_store<V>::scalar* Lval,
                  const long long* Uptr, const IDX* Ucol_in, const typename dd_store<V>::scalar* Uval, const IDX* p_in, const IDX* q_in,
                  const char* name) {
  if (!d) return fail(MG_ERR_INVALID, "null handle");
  if (d->kind != dd_store<V>::kind) {
    if (dd_store<V>::kind == 1 && d->kind == 0)
      return fail(MG_ERR_STATE, "mg_dd_set_factor_CFP64_INT64 on a handle of Float64 values (mg_dd_create_CFP64_INT64)");
    return fail(MG_ERR_STATE, "%s on a handle of %s values (%s)", name, lu_kind_name(d->kind), dd_factor_names(d->kind));
  }
  if (ic < 1 || ic > d->numSub) return fail(MG_ERR_INVALID, "sub-domain %lld outside 1..%lld", ic, d->numSub);
  if (n_i < 1 || !Lptr || !Lcol_in || !Lval || !Uptr || !Ucol_in || !Uval || !p_in || !q_in) return fail(MG_ERR_INVALID, "null or empty factor");
  mg_dd::Sub& S = d->sub[(size_t)ic - 1];
  if (n_i != S.n) return fail(MG_ERR_INVALID, "sub-domain %lld: factors of order %lld, but its index list holds %lld rows", ic, n_i, S.n);
  if (Lptr[0] != 1 || Uptr[0] != 1 || Lptr[n_i] < 1 || Uptr[n_i] < 1) return fail(MG_ERR_INVALID, "row pointers must be 1-based");
  if (Lptr[n_i] - 1 >= (1LL << 31) - 1 || Uptr[n_i] - 1 >= (1LL << 31) - 1) return fail(MG_ERR_UNSUPPORTED, "factors exceed int32 device indices");
  for (long long i = 0; i < n_i; ++i)
    if (Lptr[i + 1] < Lptr[i] || Uptr[i + 1] < Uptr[i]) return fail(MG_ERR_INVALID, "row pointers must not decrease");
  std::vector<long long> lc, uc, pp, qq;
  const long long *Lcol, *Ucol, *p, *q;
  if constexpr (std::is_same<IDX, long long>::value) {
    Lcol = Lcol_in; Ucol = Ucol_in; p = p_in; q = q_in;
  } else {
    lc.assign(Lcol_in, Lcol_in + (Lptr[n_i] - 1)); uc.assign(Ucol_in, Ucol_in + (Uptr[n_i] - 1));
    pp.assign(p_in, p_in + n_i); qq.assign(q_in, q_in + n_i);
    Lcol = lc.data(); Ucol = uc.data(); p = pp.data(); q = qq.data();
  }
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
  const size_t vw = dd_store<V>::comps;
  const size_t ln = (size_t)(Lptr[n_i] - 1), un = (size_t)(Uptr[n_i] - 1);
  DdVals<V>* W = dd_vals<V>(d);
  S.Lptr.assign(Lptr, Lptr + n_i + 1);
  S.Uptr.assign(Uptr, Uptr + n_i + 1);
  S.Lcol.assign(Lcol, Lcol + ln);
  S.Ucol.assign(Ucol, Ucol + un);
  W->Lval[(size_t)ic - 1].assign(Lval, Lval + vw * ln);
  W->Uval[(size_t)ic - 1].assign(Uval, Uval + vw * un);
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
template <typename V>
int dd_set(mg_dd* d, bool adjoint, typename DdVals<V>::Set** out, const mgk::DdSub** desc_dev) {
  typedef typename dd_store<V>::scalar T;
  typedef typename DdVals<V>::Set Set;
  DdVals<V>* W = dd_vals<V>(d);
  Set*& F = adjoint ? W->adj : W->fwd;
  DevBuf<mgk::DdSub>& DD = adjoint ? d->desc_adj : d->desc_fwd;
  if (!F) {
    UploadFence upload_fence;
    std::vector<int> Lptr, Lcol, Uptr, Ucol, P, Q, Lorder, Uorder, Llvl, Ulvl;
    std::vector<T> Lval, Uval;
    std::vector<mgk::DdSub> desc((size_t)d->numSub);
    std::vector<long long> lp, lc, up, uc;
    std::vector<T> lv, uv;
    std::vector<int> LP, LC, LO, LL, UP, UC, UO, UL;
    for (long long s = 0; s < d->numSub; ++s) {
      const mg_dd::Sub& S = d->sub[(size_t)s];
      mgk::DdSub& e = desc[(size_t)s];
      e = mgk::DdSub{};
      e.n = (int)S.n;
      e.vec0 = (int)S.idx0;
      if (S.big) continue;   // (its own applier holds its factors)
      const std::vector<long long>*pl = &S.Lptr, *cl = &S.Lcol, *pu = &S.Uptr, *cu = &S.Ucol, *pp = &S.p, *qq = &S.q;
      const std::vector<T>*vl = &W->Lval[(size_t)s], *vu = &W->Uval[(size_t)s];
      if (adjoint) {   // x[p] = L' \ (U' \ b[q]) (parLU.cpp:194-260; ' conjugates for complex values): U' takes L's place
        // (values are moved, a complex one with its sign bit flipped: exact in either precision)
        cx_adjoint_csr1<T, dd_store<V>::comps>(S.n, S.Uptr, S.Ucol, *vu, lp, lc, lv);
        cx_adjoint_csr1<T, dd_store<V>::comps>(S.n, S.Lptr, S.Lcol, *vl, up, uc, uv);
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
    Set* G = new Set();
    auto up_i = [&](DevBuf<int>& b, const std::vector<int>& v) -> int {
      MG_TRY(b.alloc(v.size()));
      if (!v.empty()) HIP_TRY(hipMemcpy(b.p, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
      return MG_OK;
    };
    auto up_d = [&](DevBuf<V>& b, const std::vector<T>& v) -> int {   // (v holds comps scalars per value)
      MG_TRY(b.alloc(v.size() / dd_store<V>::comps));
      if (!v.empty()) HIP_TRY(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
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
int dd_sweeps(mg_dd* d, hipStream_t stream, typename DdVals<T>::Set& G, const mgk::DdSub* desc_dev, const T* b, T* x, long long niter,
              bool adjoint, bool from_zero) {
  DdVals<T>* W = dd_vals<T>(d);
  mgk::DdDevT<T> D;
  D.rowptr = d->rowptr.p; D.col = d->col.p; D.val = W->val.p;
  D.idx = d->idx.p; D.sub = desc_dev; D.members = d->members.p;
  D.Lptr = G.Lptr.p; D.Lcol = G.Lcol.p; D.Lval = G.Lval.p; D.Lorder = G.Lorder.p; D.Llvl = G.Llvl.p;
  D.Uptr = G.Uptr.p; D.Ucol = G.Ucol.p; D.Uval = G.Uval.p; D.Uorder = G.Uorder.p; D.Ulvl = G.Ulvl.p;
  D.p = G.P.p; D.q = G.Q.p;
  D.r = W->r.p; D.y = W->y.p;
  T* w = W->w.p;
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
          if constexpr (!std::is_same<T, double>::value) {   // (the applier of mg_complex.inc in its instantiation for T)
            CxLuT<T>* B = mg_lu_slot<T>(S.big);
            CxLuSetT<T>* LS = nullptr;
            MG_TRY(cxlu_set(B, adjoint, &LS));
            theirs = B->stream;
            HIP_TRY(hipStreamWaitEvent(theirs, d->ev_mine, 0));
            MG_TRY(cxlu_solve_dev<T>(B, *LS, r, t, 1));
          } else {
            mg_hierarchy* h = nullptr;
            MG_TRY(lu_hierarchy(S.big, adjoint, &h));
            MG_TRY(check_ready(h, n_i, 1));   // (created for one right-hand side and private to this handle: nrhs stays 1)
            theirs = h->play->stream;
            HIP_TRY(hipStreamWaitEvent(theirs, d->ev_mine, 0));
            MG_TRY(cycle_dev(h, r, t, true));
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

// The arguments of an apply and the handle's value type (V: the entry point's)
template <typename V>
int dd_args(mg_dd* d, const void* b, const void* x, long long n, long long niter, const char* name) {
  if (!d) return fail(MG_ERR_INVALID, "null handle");
  if (d->kind != dd_store<V>::kind)
    return fail(MG_ERR_STATE, "%s on a handle of %s values (mg_dd_apply*_%s)", name, lu_kind_name(d->kind), dd_kind_sfx(d->kind));
  if (!d->finalized) return fail(MG_ERR_STATE, "%s before mg_dd_finalize", name);
  if (n != d->n) return fail(MG_ERR_INVALID, "n=%lld but the operator has order %lld", n, d->n);
  if (!b || !x || b == x || niter < 0) return fail(MG_ERR_INVALID, "bad argument (b and x must be two vectors)");
  (void)hipSetDevice(d->device);
  return MG_OK;
}

// niter sweeps on device vectors of the handle's kind V, enqueued on `stream` (no synchronisation); from_zero: from x = 0, whatever
// x holds
template <typename V>
int dd_run(mg_dd* d, hipStream_t stream, const V* b_dev, V* x_dev, long long niter, long long doTranspose, bool from_zero = false) {
  typename DdVals<V>::Set* G = nullptr;
  const mgk::DdSub* desc_dev = nullptr;
  MG_TRY(dd_set<V>(d, doTranspose != 0, &G, &desc_dev));
  return dd_sweeps<V>(d, stream, *G, desc_dev, b_dev, x_dev, niter, doTranspose != 0, from_zero);
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
// zero, or (one level only, MGcycle.jl:13-18) from the caller's x.  b, x: the hierarchy's own coarsest vectors - double or interleaved
// ComplexF64 behind double pointers, and the complex64 pairs of a CF32 hierarchy (mg_set_coarse_dd admits matching kinds only).
int dd_coarse(mg_hierarchy* h, const double* b, double* x, bool x_zero) {
  mg_dd* d = h->coarse_dd;
  if (!d->finalized) return fail(MG_ERR_STATE, "the sweep handle of the coarsest solve is not finalized (mg_dd_finalize)");
  if (d->kind == 1) return dd_run<cx_t>(d, h->play->stream, reinterpret_cast<const cx_t*>(b), reinterpret_cast<cx_t*>(x), 1, 0, x_zero);
  if (d->kind != 0) return fail(MG_ERR_STATE, "internal: a sweep handle of %s values serves no double vectors", lu_kind_name(d->kind));
  return dd_run<double>(d, h->play->stream, b, x, 1, 0, x_zero);
}
int dd_coarse(mg_hierarchy* h, const cf_t* b, cf_t* x, bool x_zero) {
  mg_dd* d = h->coarse_dd;
  if (!d->finalized) return fail(MG_ERR_STATE, "the sweep handle of the coarsest solve is not finalized (mg_dd_finalize)");
  if (d->kind != 3) return fail(MG_ERR_STATE, "internal: a sweep handle of %s values serves no complex64 vectors", lu_kind_name(d->kind));
  return dd_run<cf_t>(d, h->play->stream, b, x, 1, 0, x_zero);
}
void dd_detach(mg_hierarchy* h) {
  if (!h->coarse_dd) return;
  h->coarse_dd->owner = nullptr;
  h->coarse_dd = nullptr;
}

// b_dev, x_dev: n values of V in HBM (the entry points take them as pointers to the host scalar)
template <typename V>
int dd_apply_dev(mg_dd* d, const typename dd_store<V>::scalar* b_dev, typename dd_store<V>::scalar* x_dev, long long n, long long niter,
                 long long doTranspose, const char* name, bool from_zero = false) {
  MG_TRY(dd_args<V>(d, b_dev, x_dev, n, niter, name));
  MG_TRY(dd_behind_owner(d));
  MG_TRY(dd_run<V>(d, d->stream, reinterpret_cast<const V*>(b_dev), reinterpret_cast<V*>(x_dev), niter, doTranspose, from_zero));
  HIP_TRY(spin_sync(d->stream));
  return MG_OK;
}

template <typename V>
int dd_apply_host(mg_dd* d, const typename dd_store<V>::scalar* b, typename dd_store<V>::scalar* x, long long n, long long niter,
                  long long doTranspose, const char* name, bool from_zero = false) {
  MG_TRY(dd_args<V>(d, b, x, n, niter, name));
  DdVals<V>* W = dd_vals<V>(d);
  const size_t len = (size_t)n;   // values
  if (W->stage_b.n != len) {
    MG_TRY(W->stage_b.alloc(len));
    MG_TRY(W->stage_x.alloc(len));
  }
  MG_TRY(dd_behind_owner(d));
  HIP_TRY(hipMemcpyAsync(W->stage_b.p, b, len * sizeof(V), hipMemcpyHostToDevice, d->stream));
  if (!from_zero) HIP_TRY(hipMemcpyAsync(W->stage_x.p, x, len * sizeof(V), hipMemcpyHostToDevice, d->stream));
  MG_TRY(dd_run<V>(d, d->stream, W->stage_b.p, W->stage_x.p, niter, doTranspose, from_zero));
  HIP_TRY(hipMemcpyAsync(x, W->stage_x.p, len * sizeof(V), hipMemcpyDeviceToHost, d->stream));
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
  return dd_create<double>(device_id, n, rowptr, colA, valA, numSub, idxptr, idx, color, out);
}
int mg_dd_create_CFP64_INT64(long long device_id, long long n, const long long* rowptr, const long long* colA, const double* valA,
                             long long numSub, const long long* idxptr, const unsigned int* idx, const long long* color, mg_dd** out) {
  return dd_create<cx_t>(device_id, n, rowptr, colA, valA, numSub, idxptr, idx, color, out);
}

int mg_dd_set_factor_FP64_INT64(mg_dd* dd, long long ic, long long n_i, const long long* Lptr, const long long* Lcol, const double* Lval,
                                const long long* Uptr, const long long* Ucol, const double* Uval, const long long* p, const long long* q) {
  return dd_set_factor<double, long long>(dd, ic, n_i, Lptr, Lcol, Lval, Uptr, Ucol, Uval, p, q, "mg_dd_set_factor_FP64_INT64");
}
int mg_dd_set_factor_CFP64_INT64(mg_dd* dd, long long ic, long long n_i, const long long* Lptr, const long long* Lcol, const double* Lval,
                                 const long long* Uptr, const long long* Ucol, const double* Uval, const long long* p, const long long* q) {
  return dd_set_factor<cx_t, long long>(dd, ic, n_i, Lptr, Lcol, Lval, Uptr, Ucol, Uval, p, q, "mg_dd_set_factor_CFP64_INT64");
}

// Single handles (opt-in above this ABI: getDomainDecompositionParam(..., singleValues=True)).  The operator comes in float with
// Int64 CSR indices (the reference's AT is Int64-indexed whatever VAL is); the factors in the three forms parLU has -
// (Float32, UInt32), (ComplexF32, UInt32), (ComplexF32, Int64): column indices and permutations in the index type of the name, row
// pointers Int64 as in every form; there is no (Float32, Int64) form.  Everything is STORED in single and every residual row and
// triangular row is EVALUATED in double (mg_dd.hpp) - the single factor applier's contract, a deliberate deviation from the
// reference, which sums in VAL.
int mg_dd_create_FP32_INT64(long long device_id, long long n, const long long* rowptr, const long long* colA, const float* valA,
                            long long numSub, const long long* idxptr, const unsigned int* idx, const long long* color, mg_dd** out) {
  return dd_create<float>(device_id, n, rowptr, colA, valA, numSub, idxptr, idx, color, out);
}
int mg_dd_create_CFP32_INT64(long long device_id, long long n, const long long* rowptr, const long long* colA, const float* valA,
                             long long numSub, const long long* idxptr, const unsigned int* idx, const long long* color, mg_dd** out) {
  return dd_create<cf_t>(device_id, n, rowptr, colA, valA, numSub, idxptr, idx, color, out);
}
int mg_dd_set_factor_FP32_UINT32(mg_dd* dd, long long ic, long long n_i, const long long* Lptr, const unsigned int* Lcol, const float* Lval,
                                 const long long* Uptr, const unsigned int* Ucol, const float* Uval, const unsigned int* p,
                                 const unsigned int* q) {
  return dd_set_factor<float, unsigned int>(dd, ic, n_i, Lptr, Lcol, Lval, Uptr, Ucol, Uval, p, q, "mg_dd_set_factor_FP32_UINT32");
}
int mg_dd_set_factor_CFP32_UINT32(mg_dd* dd, long long ic, long long n_i, const long long* Lptr, const unsigned int* Lcol, const float* Lval,
                                  const long long* Uptr, const unsigned int* Ucol, const float* Uval, const unsigned int* p,
                                  const unsigned int* q) {
  return dd_set_factor<cf_t, unsigned int>(dd, ic, n_i, Lptr, Lcol, Lval, Uptr, Ucol, Uval, p, q, "mg_dd_set_factor_CFP32_UINT32");
}
int mg_dd_set_factor_CFP32_INT64(mg_dd* dd, long long ic, long long n_i, const long long* Lptr, const long long* Lcol, const float* Lval,
                                 const long long* Uptr, const long long* Ucol, const float* Uval, const long long* p, const long long* q) {
  return dd_set_factor<cf_t, long long>(dd, ic, n_i, Lptr, Lcol, Lval, Uptr, Ucol, Uval, p, q, "mg_dd_set_factor_CFP32_INT64");
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
      const size_t si = (size_t)d->members_h[(size_t)(c.m0 + m)];
      MG_TRY(dd_with(d, [&](auto* W) {
        typedef typename std::remove_pointer<decltype(W)>::type::value V;
        if constexpr (std::is_same<V, double>::value)
          return mg_lu_create_FP64_INT64(d->device, S.n, S.Lptr.data(), S.Lcol.data(), W->Lval[si].data(), S.Uptr.data(), S.Ucol.data(),
                                         W->Uval[si].data(), S.p.data(), S.q.data(), &S.big);
        else   // (the handle keeps Int64 indices whatever form the factors came in)
          return cxlu_create_entry<V, long long>(d->device, S.n, S.Lptr.data(), S.Lcol.data(), W->Lval[si].data(), S.Uptr.data(),
                                                 S.Ucol.data(), W->Uval[si].data(), S.p.data(), S.q.data(), &S.big);
      }));
      long long f[7];
      MG_TRY(mg_lu_form(S.big, 0, f));
      S.big_launches = f[1] ? f[3] + f[4] + (f[2] > 0 ? 3 : 0) + 1 : 1;   // levels, the trailing block's three kernels, the scatter
    }
  }
  MG_TRY(dd_with(d, [&](auto* W) {
    typedef typename std::remove_pointer<decltype(W)>::type::value V;
    if (wmax > 0) MG_TRY(W->w.alloc((size_t)wmax));
    typename DdVals<V>::Set* G = nullptr;
    const mgk::DdSub* desc_dev = nullptr;
    return dd_set<V>(d, false, &G, &desc_dev);
  }));
  d->finalized = true;
  return MG_OK;
}

// b, x: host vectors of n values (x in/out); niter sweeps; doTranspose reaches the sub-domain solves only (DDSerial.jl:128)
int mg_dd_apply_FP64(mg_dd* d, const double* b, double* x, long long n, long long niter, long long doTranspose) {
  return dd_apply_host<double>(d, b, x, n, niter, doTranspose, "mg_dd_apply_FP64");
}
int mg_dd_apply_CFP64(mg_dd* d, const double* b, double* x, long long n, long long niter, long long doTranspose) {
  return dd_apply_host<cx_t>(d, b, x, n, niter, doTranspose, "mg_dd_apply_CFP64");
}
int mg_dd_apply_dev_FP64(mg_dd* d, const double* b_dev, double* x_dev, long long n, long long niter, long long doTranspose) {
  return dd_apply_dev<double>(d, b_dev, x_dev, n, niter, doTranspose, "mg_dd_apply_dev_FP64");
}
int mg_dd_apply_dev_CFP64(mg_dd* d, const double* b_dev, double* x_dev, long long n, long long niter, long long doTranspose) {
  return dd_apply_dev<cx_t>(d, b_dev, x_dev, n, niter, doTranspose, "mg_dd_apply_dev_CFP64");
}

// One sweep from x = 0 (what getDDpreconditioner and the cycle's coarsest solve ask for): x is output only - it is zero-filled on
// the stream, then swept.
int mg_dd0_apply_FP64(mg_dd* d, const double* b, double* x, long long n, long long doTranspose) {
  return dd_apply_host<double>(d, b, x, n, 1, doTranspose, "mg_dd0_apply_FP64", true);
}
int mg_dd0_apply_CFP64(mg_dd* d, const double* b, double* x, long long n, long long doTranspose) {
  return dd_apply_host<cx_t>(d, b, x, n, 1, doTranspose, "mg_dd0_apply_CFP64", true);
}
int mg_dd0_apply_dev_FP64(mg_dd* d, const double* b_dev, double* x_dev, long long n, long long doTranspose) {
  return dd_apply_dev<double>(d, b_dev, x_dev, n, 1, doTranspose, "mg_dd0_apply_dev_FP64", true);
}
int mg_dd0_apply_dev_CFP64(mg_dd* d, const double* b_dev, double* x_dev, long long n, long long doTranspose) {
  return dd_apply_dev<cx_t>(d, b_dev, x_dev, n, 1, doTranspose, "mg_dd0_apply_dev_CFP64", true);
}

// the same entry points for Float32 and ComplexF32 handles: b, x in float (complex: interleaved)
int mg_dd_apply_FP32(mg_dd* d, const float* b, float* x, long long n, long long niter, long long doTranspose) {
  return dd_apply_host<float>(d, b, x, n, niter, doTranspose, "mg_dd_apply_FP32");
}
int mg_dd_apply_CFP32(mg_dd* d, const float* b, float* x, long long n, long long niter, long long doTranspose) {
  return dd_apply_host<cf_t>(d, b, x, n, niter, doTranspose, "mg_dd_apply_CFP32");
}
int mg_dd_apply_dev_FP32(mg_dd* d, const float* b_dev, float* x_dev, long long n, long long niter, long long doTranspose) {
  return dd_apply_dev<float>(d, b_dev, x_dev, n, niter, doTranspose, "mg_dd_apply_dev_FP32");
}
int mg_dd_apply_dev_CFP32(mg_dd* d, const float* b_dev, float* x_dev, long long n, long long niter, long long doTranspose) {
  return dd_apply_dev<cf_t>(d, b_dev, x_dev, n, niter, doTranspose, "mg_dd_apply_dev_CFP32");
}
int mg_dd0_apply_FP32(mg_dd* d, const float* b, float* x, long long n, long long doTranspose) {
  return dd_apply_host<float>(d, b, x, n, 1, doTranspose, "mg_dd0_apply_FP32", true);
}
int mg_dd0_apply_CFP32(mg_dd* d, const float* b, float* x, long long n, long long doTranspose) {
  return dd_apply_host<cf_t>(d, b, x, n, 1, doTranspose, "mg_dd0_apply_CFP32", true);
}
int mg_dd0_apply_dev_FP32(mg_dd* d, const float* b_dev, float* x_dev, long long n, long long doTranspose) {
  return dd_apply_dev<float>(d, b_dev, x_dev, n, 1, doTranspose, "mg_dd0_apply_dev_FP32", true);
}
int mg_dd0_apply_dev_CFP32(mg_dd* d, const float* b_dev, float* x_dev, long long n, long long doTranspose) {
  return dd_apply_dev<cf_t>(d, b_dev, x_dev, n, 1, doTranspose, "mg_dd0_apply_dev_CFP32", true);
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
  // the handle's kind must be the hierarchy's: Float64, ComplexF64, or ComplexF32 on a CF32 handle (the sweep then runs on the cycle's
  // own complex64 coarsest vectors, no widened pair).  A ComplexF64 sweep on a CF32 handle stays unserved.
  const int hk = !h->cx ? 0 : h->cx->single ? 3 : 1;
  if (hk == 3 && d->kind == 1) return fail(MG_ERR_UNSUPPORTED, "a Schwarz sweep as coarsest solve is not served for CF32 handles");
  if (d->kind != hk)
    return fail(MG_ERR_STATE, "mg_set_coarse_dd: a sweep handle of %s values on a hierarchy of %s values", lu_kind_name(d->kind), lu_kind_name(hk));
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

// info[0..6): value type (0 Float64, 1 ComplexF64, 2 Float32, 3 ComplexF32); sub-domains; colours present; colours run batched; colours run in
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
  info[0] = d->kind;
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
  // (any kind: b_dev and x_dev hold the handle's values, whatever the pointer type says)
  auto run = [&](long long niter) {
    return dd_with(d, [&](auto* W) {
      typedef typename std::remove_pointer<decltype(W)>::type::value V;
      return dd_run<V>(d, d->stream, reinterpret_cast<const V*>(b_dev), reinterpret_cast<V*>(x_dev), niter, doTranspose);
    });
  };
  MG_TRY(dd_with(d, [&](auto* W) {
    return dd_args<typename std::remove_pointer<decltype(W)>::type::value>(d, b_dev, x_dev, n, 0, "mg_dd_time_dev");
  }));
  MG_TRY(dd_behind_owner(d));
  MG_TRY(run(0));   // the direction's set is built before the first sample
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = MG_OK;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) rc = fail(MG_ERR_HIP, "hipEventCreate failed");
  for (long long it = 0; it < warmup + reps && rc == MG_OK; ++it) {
    if (hipEventRecord(e0, d->stream) != hipSuccess) rc = fail(MG_ERR_HIP, "hipEventRecord failed");
    if (rc == MG_OK) rc = run(1);
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
  delete d->vd; delete d->vz; delete d->vs; delete d->vc;
  delete d;
  return MG_OK;
}

}  // extern "C"
