"""Crafted triples (R, A, P, pattern of C) for the numeric Galerkin kernels and the relaxation vectors of the device re-setup
(rap_numeric in csrc/mg_kernels.hpp; cx_rap_numeric<d2_t, double> and <f2_t, float> in csrc/mg_complex.hpp; relax_jacobi,
colsumsq_kernel, relax_spai and their cx_* forms).  numpy / scipy only: tests/test_rap_crafted_host.py runs the checks of this file
against plain restatements of the kernels and against wrong variants of them, tests/test_rap_crafted_gpu.py against the device.

The hierarchy (hierarchy()): three hand-assembled levels of 9000, 5000 and 40 rows; the third only closes the hierarchy and makes
level 2 -> 3 a second product, whose A is what the device computed for level 2.  One set of patterns serves the three value types
(VTYPES): float64; complex128 (A complex, P and R real); complex64 (every input rounded to single once, references from the rounded
data).  The pattern of a coarse operator is the structural pattern of R A P with sorted rows plus the unreachable entries below.

What the rows contain (asserted by hierarchy(); `marks` names the rows):
  rows of P    exactly 0, 1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 129 entries (P_LENS): one lane trip and the first entry of the next for lane
               group widths 64, 32, 8, 4 - each reached from a row of A that a row of R reaches;
  rows of C    exactly 0, 1, 2, 2047, 2048, 2049, 4097 entries (C_LENS): one, two and three chunks of the real RAP_CAP = 2048; every
               column of the 2049- and 4097-entry rows is reached, so the first and last column of every chunk carry terms (the cmin /
               cmax skip, both ends of the binary search);
  empty rows   an empty row of R whose row of C holds three structural entries (they must come back exactly 0.0); rows of A that are
               empty and reached from R; rows of P that are empty and reached from A; an empty row of R on level 2 -> 3 as well;
  unreachable  a 4100-entry row of C whose entries 0, 2047, 2048 and 4099 (start, both sides of the chunk boundary, end) no term
               reaches, and two more in every 16th ordinary row (chunk boundaries of rap_chunk = 1 and 10);
  stored order the crafted rows of R and of A and every 8th ordinary row of both are stored in an order that is not ascending (the
               kernels walk the stored order; only C's rows must be sorted).  The upload accepts them: nothing checks R or A;
  magnitudes   every column c of P is scaled by 2^s(c), s uniform in [-30, 30] (level 2 -> 3: [-8, 8]), so every row of C spans up
               to 2^60: a bound relative to the largest entry would hide a wrong small one;
  cancellation row `cancel` holds one entry whose two terms cancel exactly and one whose terms cancel to 2^-40 of their magnitudes
               (complex64: 1 + 2^-40 rounds to 1, both cancel exactly);
  relaxation   level 1: the diagonal stored first, last and in the middle of its row, one row that is its diagonal alone, columns
               of exactly 1, 2, 64, 65 and 3000 entries (COL_LENS).
Two families of values on these patterns: "crafted" (seeded normal values, the scalings and cancellations above) and "exact"
(R, P in {+-1, +-2, +-0.5}, A likewise or in {+-1, +-i}): every partial sum of the exact family is a multiple of 2^-6 far below
2^53, so every entry of C must equal the exact product bit for bit; values() asserts that the level-2 sums also fit a single
(those of level 3 do as well: the exact comparison of the complex64 results on the host and on the device shows it).

Reference and bound, entry by entry, no entry left out.  The terms of entry (i, c) are t = r_ik a_kj p_jc over all (k, j) (Terms:
the index lists, in the kernels' walk order).  ref = sum t in np.longdouble (64-bit significand: its own error, 2^-64 per operation,
is 2^-11 of the smallest bound below), from the finer level's values AS THE DEVICE HOLDS THEM, so that no tolerance propagates from
level 1 -> 2 into level 2 -> 3.  With m terms, u = 2^-53 and gamma(k) = k u / (1 - k u):
  float64     |got - ref| <= gamma(m + 2) sum|t|.  A term passes through two multiplications ((r a), then times p) and the sum of m
              terms through at most m - 1 additions - a fused multiply-add only removes roundings -, so (1 + u)^(m + 1) covers
              every path through the sum; one further unit covers second order (the convention of default_paths_check.py).
  complex128  the same with u_c = 2 sqrt(2) u (complex_awkward_cases.gamma: it covers a full complex product; here a real times a
              complex needs less) and the count m + groups + 1: the `groups` copies of the accumulator are added in group order
              at the end (groups - 1 more additions; lane_groups() restates how the host picks the count).  |.| is the modulus.
  complex64   the kernel forms the complex128 sum s and rounds each part once on the store: per part
              |got - ref| <= B + 2^-24 (|ref part| + B), B the complex128 bound.
  m = 0       sum|t| = 0: the entry must be exactly zero, whatever it held before (the GPU tests fill C with NaN first).
A perturbation of 2^-40 relative in one entry leaves the bound while gamma(m + 2) sum|t| < 2^-40 |ref|: with no cancellation that is
m + 2 < 2^13, so from m = 8190 terms on (complex: m + groups + 1 >= 2896) this check cannot see it.

Relaxation vectors, bit for bit (jacobi(), spai()): Jac d_i = omega / a_ii, one correctly rounded division (a_ii the LAST stored
entry of row i in column i, 0 without one); SPAI s_j = the sum over column j in ascending row order of the ROUNDED squares
(colsumsq_kernel and cx_colsumsq switch contraction off), d_i = omega * (a_ii / s_i).  Complex: Jac is cx_jac_div (csrc/mg_complex.hpp), contraction
off: s = fl(fl(x x) + fl(y y)), d = (fl(fl(omega x) + fl(0 y)) / s, fl(fl(0 x) - fl(omega y)) / s); SPAI is (omega (x / s_i),
omega (-y / s_i)) with s_j the sum of the rounded re^2 + im^2; complex64 rounds each part once on the store.  Compared bit for bit,
the sign of a zero included; only NaN (0 / 0 on a row without diagonal in an empty column) equals any NaN, whose sign and payload
are the processor's choice.  An entry of C that no term reaches must be +0.0, not -0.0; the exact family is compared by value (an
exact sum that cancels is +0.0 on the device and in the reference alike)."""
import hashlib

import numpy as np
import scipy.sparse as sp

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the reference needs an 80-bit (or wider) long double"
U = 2.0 ** -53
U32 = 2.0 ** -24
RAP_CAP = 2048                 # csrc/mg_kernels.hpp
CX_RAP_GROUPS = 8              # csrc/mg_complex.hpp: lane groups unless the option rap_groups says otherwise
N1, N2, N3 = 9000, 5000, 40
G1, G2 = 2000, 16              # first ordinary fine row / coarse row: the crafted rows lie below
P_LENS = (0, 1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 129)
C_LENS = (0, 1, 2, 2047, 2048, 2049, 4097)
COL_LENS = {2010: 1, 2011: 2, 2012: 64, 2013: 65, 2014: 3000}     # column of level 1's A -> its number of entries
DIAG_ROWS = {"first": 3000, "last": 3001, "middle": 3002, "alone": 3003}
VTYPES = ("float64", "complex128", "complex64")
OMEGA = 0.8


def gamma(k, u=U):
    k = np.asarray(k, dtype=np.float64)
    return k * u / (1.0 - k * u)


def gamma_c(k, u=U):
    """complex_awkward_cases.gamma: u_c = 2 sqrt(2) u."""
    return gamma(k, 2.0 * np.sqrt(2.0) * u)


def lane_groups(requested, rap_chunk, max_row):
    """The lane groups cx_rap uses for a level whose longest row of C has max_row entries (csrc/mg_complex.inc): the largest
    power of two <= min(requested or 8, 16), halved while chunk * (16 groups + 4) bytes exceed 32 KB."""
    cap = max(1, min(int(rap_chunk), RAP_CAP))
    chunk = max(1, min(cap, int(max_row)))
    want = min(int(requested) if requested and requested > 0 else CX_RAP_GROUPS, 16)
    g = 1
    while g * 2 <= want:
        g *= 2
    while g > 1 and chunk * (g * 16 + 4) > 32768:
        g //= 2
    return g


class Pattern:
    """A CSR pattern whose rows keep their stored order."""

    def __init__(self, rows, ncols):
        lens = np.array([len(r) for r in rows], dtype=np.int64)
        self.indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.indices = (np.concatenate([np.asarray(r, dtype=np.int64) for r in rows if len(r)]) if self.indptr[-1]
                        else np.empty(0, dtype=np.int64))
        self.shape = (len(rows), int(ncols))
        self.nnz = int(self.indptr[-1])
        self.rows = np.repeat(np.arange(len(rows), dtype=np.int64), lens)
        self.lens = lens
        for r in rows:
            assert len(np.unique(r)) == len(r) and (len(r) == 0 or (min(r) >= 0 and max(r) < ncols))

    @classmethod
    def of(cls, M):
        M = sp.csr_matrix(M)
        M.sort_indices()
        return cls([M.indices[M.indptr[i]:M.indptr[i + 1]] for i in range(M.shape[0])], M.shape[1])

    def csr(self, data):
        data = np.asarray(data)
        assert data.shape == (self.nnz,)
        return sp.csr_matrix((data.copy(), self.indices.astype(np.int32), self.indptr.astype(np.int32)), shape=self.shape)

    def ones(self):
        return sp.csr_matrix((np.ones(self.nnz), self.indices.copy(), self.indptr.copy()), shape=self.shape)

    def find(self, i, c):
        s, e = self.indptr[i], self.indptr[i + 1]
        k = np.flatnonzero(self.indices[s:e] == c)
        assert k.size == 1, (i, c)
        return int(s + k[0])

    def unsorted_rows(self):
        """Rows whose stored columns do not ascend."""
        bad = np.zeros(self.shape[0], dtype=bool)
        if self.nnz > 1:
            same = self.rows[1:] == self.rows[:-1]
            bad[self.rows[1:][same & (np.diff(self.indices) < 0)]] = True
        return bad


class Terms:
    """The product terms of C = R A P on C's pattern: ir, ia, ip index the values of R, A, P of every term, pos its entry of C;
    sorted by entry, the kernels' walk order (R stored order, A stored order, P stored order) kept inside an entry.  goff: the
    offset of the A entry in its row (the lane group of cx_rap_numeric is goff % groups), poff: of the P entry in its row."""

    def __init__(self, R, A, P, C):
        assert R.shape[1] == A.shape[0] and A.shape[1] == P.shape[0] and C.shape == (R.shape[0], P.shape[1])
        rk = R.indices
        lenA = A.lens[rk]
        e_r = np.repeat(np.arange(R.nnz, dtype=np.int64), lenA)
        off = np.arange(int(lenA.sum()), dtype=np.int64) - np.repeat(np.cumsum(lenA) - lenA, lenA)
        e_a = np.repeat(A.indptr[rk], lenA) + off
        j = A.indices[e_a]
        lenP = P.lens[j]
        ir, ia = np.repeat(e_r, lenP), np.repeat(e_a, lenP)
        poff = np.arange(int(lenP.sum()), dtype=np.int64) - np.repeat(np.cumsum(lenP) - lenP, lenP)
        ip = np.repeat(P.indptr[j], lenP) + poff
        key = R.rows[ir] * C.shape[1] + P.indices[ip]
        ckey = C.rows * C.shape[1] + C.indices
        assert (np.diff(ckey) > 0).all(), "the rows of C must be sorted"
        pos = np.searchsorted(ckey, key)
        assert pos.size == 0 or (pos.max() < ckey.size and (ckey[pos] == key).all()), "the pattern of C misses a reachable column"
        o = np.argsort(pos, kind="stable")
        self.ir, self.ia, self.ip, self.pos, self.poff = ir[o], ia[o], ip[o], pos[o], poff[o]
        self.goff = (e_a - A.indptr[A.rows[e_a]])[np.repeat(np.arange(e_a.size), lenP)][o]
        self.nnz = C.nnz
        self.m = np.bincount(self.pos, minlength=C.nnz).astype(np.int64)
        self.C = C
        self.hit = np.flatnonzero(self.m > 0)
        self.starts = (np.cumsum(self.m) - self.m)[self.hit]
        self.entry_rows, self.entry_cols = C.rows, C.indices

    def name(self, e):
        return f"entry ({int(self.entry_rows[e])}, {int(self.entry_cols[e])}) [{int(e)}], {int(self.m[e])} terms"


def _wide(v):
    v = np.asarray(v)
    return v.astype(np.complex128) if np.iscomplexobj(v) else v.astype(np.float64)


def reference(T, Rv, Av, Pv):
    """(ref_re, ref_im) in long double and sum|t| in double, per entry of C (zeros where no term arrives)."""
    rp = _wide(Rv)[T.ir].astype(LD) * _wide(Pv)[T.ip].astype(LD)
    a = _wide(Av)[T.ia]
    re = np.zeros(T.nnz, dtype=LD)
    im = np.zeros(T.nnz, dtype=LD)
    sab = np.zeros(T.nnz, dtype=np.float64)
    if T.pos.size:
        re[T.hit] = np.add.reduceat(rp * a.real.astype(LD), T.starts)
        if np.iscomplexobj(a):
            im[T.hit] = np.add.reduceat(rp * a.imag.astype(LD), T.starts)
        sab[T.hit] = np.add.reduceat(np.abs(rp) * np.abs(a).astype(LD), T.starts).astype(np.float64) * (1.0 + 2.0 ** -50)
    return re, im, sab


def bound(vt, T, ref, groups=1):
    """The entry bound of the module docstring: B (float64, complex128: on the modulus), or the pair of per-part bounds (complex64)."""
    re, im, sab = ref
    if vt == "float64":
        return gamma(T.m + 2) * sab
    B = gamma_c(T.m + groups + 1) * sab
    if vt == "complex128":
        return B
    return (B + U32 * (np.abs(re).astype(np.float64) + B), B + U32 * (np.abs(im).astype(np.float64) + B))


def check_entries(name, vt, T, got, ref, groups=1, exact=False):
    """Every entry of `got` (C's values in stored order) against ref within bound(); returns the largest share of a bound used.
    exact: every entry must equal the reference as a value (the exact family)."""
    got = np.asarray(got)
    assert got.shape == (T.nnz,) and got.dtype == np.dtype(vt), (got.shape, got.dtype)
    re, im, sab = ref
    g = _wide(got)
    dre, dim = np.abs(g.real.astype(LD) - re), np.abs((g.imag if np.iscomplexobj(g) else np.zeros(T.nnz)).astype(LD) - im)
    bd = bound(vt, T, ref, groups)
    minus = (T.m == 0) & (np.signbit(g.real) | (np.signbit(g.imag) if np.iscomplexobj(g) else False))
    if minus.any():        # an entry no term reaches is the accumulator's initial +0.0, bit for bit
        raise AssertionError(f"{name}: {T.name(int(np.flatnonzero(minus)[0]))} is -0.0, not 0.0")
    if exact:
        bad = ~((dre == 0) & (dim == 0))
        share = np.where(bad, np.inf, 0.0)
    elif vt == "complex64":
        bad = ~((dre <= bd[0]) & (dim <= bd[1]))
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.maximum(np.where(bd[0] > 0, (dre / np.where(bd[0] > 0, bd[0], 1)).astype(np.float64), 0.0),
                               np.where(bd[1] > 0, (dim / np.where(bd[1] > 0, bd[1], 1)).astype(np.float64), 0.0))
        bd = bd[0]
    else:
        err = np.hypot(dre, dim) if vt != "float64" else dre
        bad = ~(err <= bd)
        share = np.where(bd > 0, (err / np.where(bd > 0, bd, 1)).astype(np.float64), 0.0)
    if bad.any():
        e = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {T.nnz} entries outside their bound; first {T.name(e)}: got {got[e]!r}, "
                             f"reference ({float(re[e])!r}, {float(im[e])!r}), bound {float(bd[e])!r}, sum|t| {sab[e]!r}")
    return float(share.max()) if share.size else 0.0


def outside(vt, T, got, ref, groups=1):
    """The entries of `got` outside their bound (what check_entries would report), as indices."""
    re, im, _ = ref
    g = _wide(np.asarray(got))
    dre, dim = np.abs(g.real.astype(LD) - re), np.abs((g.imag if np.iscomplexobj(g) else np.zeros(T.nnz)).astype(LD) - im)
    bd = bound(vt, T, ref, groups)
    if vt == "complex64":
        return np.flatnonzero(~((dre <= bd[0]) & (dim <= bd[1])))
    return np.flatnonzero(~((np.hypot(dre, dim) if vt != "float64" else dre) <= bd))


def _sequential(keys, nkeys, t):
    """acc[k] = the terms of key k added one after the other in the order given (double or complex128 arithmetic)."""
    acc = np.zeros(nkeys, dtype=t.dtype)
    if keys.size == 0:
        return acc
    o = np.argsort(keys, kind="stable")
    k, tt = keys[o], t[o]
    cnt = np.bincount(k, minlength=nkeys)
    rank = np.arange(k.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    o2 = np.argsort(rank, kind="stable")
    k, tt, rank = k[o2], tt[o2], rank[o2]
    cuts = np.concatenate([[0], np.cumsum(np.bincount(rank))])
    for s in range(cuts.size - 1):
        sel = slice(cuts[s], cuts[s + 1])
        acc[k[sel]] = acc[k[sel]] + tt[sel]           # (one term per key in a round: no index repeats)
    return acc


def kernel_order(vt, T, Rv, Av, Pv, groups=1, weight=None, pos=None, first_trip=None, skip_group=None):
    """A plain restatement of the product in the kernels' order: R in stored order, A in stored order (entry q of a row of A is
    lane group q % groups'), one row of P per step, every entry's terms added one after the other into its group's copy, the
    copies summed in group order; double / complex128 arithmetic, unfused; complex64: widened inputs, one rounding at the end.
    The wrong variants of tests/test_rap_crafted_host.py: weight (a factor per term: 0 drops it, 2 adds it twice), pos (other target
    entries), first_trip = W (the entries of a row of P beyond the first W dropped), skip_group (that copy is not summed)."""
    if vt == "float64":
        groups = 1
    ra = _wide(Rv)[T.ir] * _wide(Av)[T.ia]
    t = ra * _wide(Pv)[T.ip]
    if weight is not None:
        t = t * weight
    if first_trip is not None:
        t = np.where(T.poff < first_trip, t, 0.0)
    p = T.pos if pos is None else pos
    acc = _sequential(p * groups + T.goff % groups, T.nnz * groups, t).reshape(T.nnz, groups)
    s = acc[:, 0].copy() if skip_group != 0 else np.zeros(T.nnz, dtype=acc.dtype)
    for q in range(1, groups):
        if q != skip_group:
            s = s + acc[:, q]
    return s.astype(np.dtype(vt))


# ---- relaxation vectors -----------------------------------------------------------------------------------------------------
def _diag(pat, val):
    """a_ii as relax_jacobi finds it: the last stored entry of row i in column i, 0 without one."""
    d = np.zeros(pat.shape[0], dtype=_wide(val).dtype)
    hit = np.flatnonzero(pat.indices == pat.rows)
    d[pat.rows[hit]] = _wide(val)[hit]             # (ascending entry index: the last one wins)
    return d


def _store(vt, re, im=None):
    if vt == "float64":
        return re
    z = np.empty(np.shape(re), dtype=np.complex128)       # (part by part: re + 1j * im would lose the sign of a zero)
    z.real, z.imag = re, im
    return z.astype(np.complex64) if vt == "complex64" else z


def jacobi(vt, pat, val, omega=OMEGA):
    """`omega / a_ii` as the kernels document it (a list of one): real one division; complex cx_jac_div, contraction off:
    s = fl(fl(x x) + fl(y y)), d = (fl(fl(omega x) + fl(0 y)) / s, fl(fl(0 x) - fl(omega y)) / s), rounded to single on the store."""
    a = _diag(pat, val)
    with np.errstate(divide="ignore", invalid="ignore"):
        if vt == "float64":
            return [omega / a]
        x, y = a.real.copy(), a.imag.copy()
        s = x * x + y * y
        return [_store(vt, (omega * x + 0.0 * y) / s, (0.0 * x - omega * y) / s)]


def colsumsq(vt, pat, val, over_rows=False):
    """s_j: the rounded squares of column j added in ascending row order (over_rows: the wrong variant that sums row i)."""
    v = _wide(val)
    sq = (v.real * v.real + v.imag * v.imag) if np.iscomplexobj(v) else v * v
    return _sequential(pat.rows if over_rows else pat.indices, pat.shape[0] if over_rows else pat.shape[1], sq)


def spai(vt, pat, val, omega=OMEGA, conj=True, over_rows=False):
    """omega * (a_ii / s_i), complex: (omega (x / s_i), omega (-y / s_i)); conj=False and over_rows=True are the wrong variants."""
    a, s = _diag(pat, val), colsumsq(vt, pat, val, over_rows)
    with np.errstate(divide="ignore", invalid="ignore"):
        if vt == "float64":
            return omega * (a / s)
        return _store(vt, omega * (a.real / s), omega * ((-a.imag if conj else a.imag) / s))


def _same_parts(g, w):
    return ((g == w) & (np.signbit(g) == np.signbit(w))) | (np.isnan(g) & np.isnan(w))


def same_values(got, want):
    """Equal bit for bit, part by part, the sign of a zero included; only a NaN equals any NaN (0 / 0 gives a NaN whose sign and
    payload are the processor's choice: x86 sets the sign bit, the GPU does not)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    parts = [(got.real, want.real), (got.imag, want.imag)] if np.iscomplexobj(got) else [(got, want)]
    return all(bool(_same_parts(g, w).all()) for g, w in parts)


def check_relax(name, vt, kind, pat, val, got, omega=OMEGA):
    """got = the device's relaxation vector of the level whose operator holds `val` (kind 0 Jac, 1 SPAI)."""
    cands = jacobi(vt, pat, val, omega) if kind == 0 else [spai(vt, pat, val, omega)]
    got = np.asarray(got)
    if any(same_values(got, c) for c in cands):
        return
    c = cands[0]
    parts = [(got.real, c.real), (got.imag, c.imag)] if np.iscomplexobj(got) else [(got, c)]
    bad = np.flatnonzero(~np.logical_and.reduce([_same_parts(g, w) for g, w in parts]))
    raise AssertionError(f"{name}: {'Jac' if kind == 0 else 'SPAI'} vector differs from the documented expression in {bad.size} of "
                         f"{got.size} rows ; first row {int(bad[0])}: got {got[bad[0]]!r}, expected {c[bad[0]]!r}")


# ---- the hierarchy ----------------------------------------------------------------------------------------------------------
_CYCLE = (129, 65, 64, 63, 9, 8, 7, 5, 4, 3, 1, 0)


def _build():
    rng = np.random.default_rng(20260611)
    Rrow = [np.empty(0, dtype=np.int64) for _ in range(N2)]
    Arow = [np.empty(0, dtype=np.int64) for _ in range(N1)]
    Prow = [np.empty(0, dtype=np.int64) for _ in range(N1)]
    extra = {}                 # coarse row -> unreachable structural columns
    marks = {}
    nxt = {"k": 10, "j": 300}

    def take(what, n=1):
        v = nxt[what]
        nxt[what] += n
        return v

    # crafted coarse rows
    marks["empty_R"] = 0
    extra[0] = np.array([3, 700, N2 - 1])
    marks["empty_A"] = 1
    Rrow[1] = np.array([1, 0])                                  # rows 0 and 1 of A stay empty: row 1 of C has no entry
    marks["one"] = 2
    Rrow[2], Arow[2] = np.array([2]), np.array([201, 200])      # row 201 of P stays empty: reached from A
    Prow[200] = np.array([40])
    marks["two"] = 3
    Rrow[3], Arow[3] = np.array([3]), np.array([203, 202])
    Prow[202], Prow[203] = np.array([41]), np.array([4000])
    marks["cancel"] = 9
    Rrow[9] = np.array([5, 4])
    Arow[4], Arow[5] = np.array([250, 251]), np.array([251, 250])
    Prow[250], Prow[251] = np.array([50]), np.array([51])

    def long_row(i, total, holes=()):
        cols = np.sort(np.concatenate([[0, N2 - 1], 1 + rng.choice(N2 - 2, total - 2, replace=False)]))
        hole = np.array(sorted(holes), dtype=np.int64)
        extra[i] = cols[hole]
        reach = rng.permutation(np.delete(cols, hole))
        js, at, c = [], 0, 0
        while at < reach.size:
            n = min(_CYCLE[c % len(_CYCLE)], reach.size - at)
            c += 1
            j = take("j")
            piece = reach[at:at + n]
            Prow[j] = piece if c % 3 == 0 else np.sort(piece)
            js.append(j)
            at += n
        js = np.array(js)
        ka, kb = take("k"), take("k")
        half = js.size // 2
        Arow[ka] = rng.permutation(js[:half])
        Arow[kb] = rng.permutation(np.concatenate([js[half:], js[:6]]))     # six rows of P reached twice: entries of two terms
        Rrow[i] = np.array([kb, ka])                                        # (stored order not ascending)

    for i, total in ((4, 2047), (5, 2048), (6, 2049), (7, 4097)):
        long_row(i, total)
        marks[f"len{total}"] = i
    long_row(8, 4100, holes=(0, 2047, 2048, 4099))
    marks["holes"] = 8
    assert nxt["k"] <= 200 and nxt["j"] <= G1
    # ordinary rows: local stencils, the fine index scaled to the coarse one
    reserved = set(COL_LENS)
    special_diag = set(DIAG_ROWS.values())
    for k in range(G1, N1):
        offs = rng.choice(np.concatenate([np.arange(-40, 0), np.arange(1, 41)]), int(rng.integers(2, 7)), replace=False)
        cols = np.unique(np.clip(k + offs, G1, N1 - 1))
        cols = np.array([c for c in cols if c != k and c not in reserved], dtype=np.int64)
        Arow[k] = np.sort(np.concatenate([cols, [k]]))
    Arow[DIAG_ROWS["first"]] = np.concatenate([[3000], np.sort(Arow[3000][Arow[3000] != 3000])[::-1]])
    Arow[DIAG_ROWS["last"]] = np.concatenate([np.sort(Arow[3001][Arow[3001] != 3001])[::-1], [3001]])
    oth = Arow[3002][Arow[3002] != 3002]
    Arow[DIAG_ROWS["middle"]] = np.concatenate([oth[oth > 3002], [3002], oth[oth < 3002]])
    Arow[DIAG_ROWS["alone"]] = np.array([3003])
    pool = np.array([k for k in range(2100, N1) if k not in special_diag], dtype=np.int64)
    for col, n in COL_LENS.items():
        for k in rng.choice(pool, n - 1, replace=False):
            Arow[k] = np.sort(np.concatenate([Arow[k], [col]]))
    for k in range(G1 + 5, N1, 8):
        if k not in special_diag and len(Arow[k]) > 1:
            Arow[k] = Arow[k][::-1].copy()
    for j in range(G1, N1):
        n = int(rng.choice(5, p=[0.03, 0.3, 0.3, 0.2, 0.17]))
        centre = G2 + (j - G1) * (N2 - G2) // (N1 - G1)
        Prow[j] = np.unique(np.clip(centre + rng.choice(np.arange(-3, 4), n, replace=False), 0, N2 - 1))
    for i in range(G2, N2):
        centre = G1 + (i - G2) * (N1 - G1) // (N2 - G2)
        ks = np.unique(np.clip(centre + rng.choice(np.arange(-6, 7), int(rng.integers(4, 9)), replace=False), G1, N1 - 1))
        Rrow[i] = ks[::-1].copy() if i % 8 == 3 else ks
    Rrow[G2] = np.array([3003, 3001, 3002, 3000, 2014, 2010])
    R1, A1, P1 = Pattern(Rrow, N1), Pattern(Arow, N1), Pattern(Prow, N2)
    S = (R1.ones() @ A1.ones() @ P1.ones()).tocsr()
    for i in range(G2 + 7, N2, 16):            # two unreachable entries in every 16th ordinary row
        free = np.setdiff1d(np.arange(max(0, i - 40), min(N2, i + 40)), S.indices[S.indptr[i]:S.indptr[i + 1]])
        extra[i] = free[[0, free.size // 2]]
    E = sp.csr_matrix((np.ones(sum(len(v) for v in extra.values())), (np.repeat(list(extra), [len(v) for v in extra.values()]),
                                                                      np.concatenate(list(extra.values())))), shape=S.shape)
    C2 = Pattern.of(S + E)
    # level 2 -> 3
    R2row = [np.sort(rng.choice(N2, int(rng.integers(40, 90)), replace=False)) for _ in range(N3)]
    R2row[0] = np.unique(np.concatenate([R2row[0], np.arange(0, 10)]))[::-1].copy()       # reaches every crafted row of level 2
    R2row[5] = np.empty(0, dtype=np.int64)
    marks["empty_R2"] = 5
    P2row = [np.sort(rng.choice(N3, int(rng.integers(0, 4)), replace=False)) for _ in range(N2)]
    R2, P2 = Pattern(R2row, N2), Pattern(P2row, N3)
    S3 = (R2.ones() @ C2.ones() @ P2.ones()).tocsr()
    E3 = sp.csr_matrix((np.ones(3), ([5, 5, 5], [0, 20, N3 - 1])), shape=S3.shape)
    C3 = Pattern.of(S3 + E3)
    H = dict(R=[R1, R2], A=[A1, C2], P=[P1, P2], C=[C2, C3], marks=marks, extra=extra,
             T=[Terms(R1, A1, P1, C2), Terms(R2, C2, P2, C3)])
    _assert_shapes(H)
    return H


def _assert_shapes(H):
    R1, A1, P1, C2, T1 = H["R"][0], H["A"][0], H["P"][0], H["C"][0], H["T"][0]
    reached = np.zeros(N1, dtype=bool)
    reached[A1.indices[np.unique(T1.ia)]] = True                          # rows of P that carry a term ...
    a_reached = np.zeros(N1, dtype=bool)
    a_reached[R1.indices] = True
    p_from_a = np.zeros(N1, dtype=bool)
    p_from_a[A1.indices[a_reached[A1.rows]]] = True                       # ... or (empty ones) are reached from a reached row of A
    for n in P_LENS:
        assert ((P1.lens == n) & (reached if n else p_from_a)).any(), f"no reached row of P with {n} entries"
    for n in C_LENS:
        assert (C2.lens == n).any(), f"no row of C with {n} entries"
    m = H["marks"]
    assert R1.lens[m["empty_R"]] == 0 and C2.lens[m["empty_R"]] == 3 and C2.lens[m["empty_A"]] == 0 and (A1.lens[[0, 1]] == 0).all()
    assert P1.lens[201] == 0 and C2.lens[m["one"]] == 1 and C2.lens[m["two"]] == 2 and C2.lens[m["holes"]] == 4100
    s = C2.indptr[m["holes"]]
    assert (T1.m[s + np.array([0, 2047, 2048, 4099])] == 0).all() and (T1.m[s + np.array([1, 2046, 2049, 4098])] > 0).all()
    for name in ("len2049", "len4097"):
        s, e = C2.indptr[m[name]], C2.indptr[m[name] + 1]
        assert (T1.m[s:e] > 0).all() and (T1.m[s:e] > 1).any()
    assert (T1.m == 0).sum() >= 300 and R1.unsorted_rows().sum() > 500 and A1.unsorted_rows().sum() > 500
    assert not C2.unsorted_rows().any() and not H["C"][1].unsorted_rows().any()
    cols = np.bincount(A1.indices, minlength=N1)
    assert all(cols[c] == n for c, n in COL_LENS.items())
    for where, k in DIAG_ROWS.items():
        row = A1.indices[A1.indptr[k]:A1.indptr[k + 1]]
        at = int(np.flatnonzero(row == k)[0])
        assert {"first": at == 0 and row.size > 2, "last": at == row.size - 1 and row.size > 2,
                "middle": 0 < at < row.size - 1, "alone": row.size == 1}[where], (where, row)
    assert H["R"][1].lens[m["empty_R2"]] == 0 and H["C"][1].lens[m["empty_R2"]] == 3


_H = None


def hierarchy():
    """The patterns, the term lists and the named rows, built once."""
    global _H
    if _H is None:
        _H = _build()
    return _H


def rdtype(vt):
    return np.float32 if vt == "complex64" else np.float64


_EXACT = np.array([1.0, -1.0, 2.0, -2.0, 0.5, -0.5])
_VALUES = {}


def values(vt, family, seed=0):
    """dict(R=[R1, R2], A=A1, P=[P1, P2]) of value arrays in stored order; family "crafted" or "exact" (module docstring).
    seed: another draw of the same family (the repeated refresh on other values)."""
    key = (vt, family, seed)
    if key in _VALUES:
        return _VALUES[key]
    H = hierarchy()
    rng = np.random.default_rng([7, {"crafted": 1, "exact": 2}[family], seed])
    cx = vt != "float64"
    R1, A1, P1, R2, P2 = H["R"][0], H["A"][0], H["P"][0], H["R"][1], H["P"][1]
    if family == "exact":
        r1, p1, r2, p2 = (rng.choice(_EXACT, M.nnz) for M in (R1, P1, R2, P2))
        a1 = rng.choice(np.array([1, -1, 1j, -1j]), A1.nnz) if cx else rng.choice(_EXACT, A1.nnz)
    else:
        r1, r2 = rng.standard_normal(R1.nnz), rng.standard_normal(R2.nnz)
        p1 = rng.standard_normal(P1.nnz) * np.exp2(rng.integers(-30, 31, N2))[P1.indices]
        p2 = rng.standard_normal(P2.nnz) * np.exp2(rng.integers(-8, 9, N3))[P2.indices]
        a1 = rng.standard_normal(A1.nnz) + (1j * rng.standard_normal(A1.nnz) if cx else 0.0)
        dg = np.flatnonzero(A1.indices == A1.rows)
        a1[dg] = (4.0 + np.abs(rng.standard_normal(dg.size))) * ((1.0 + 0.25j) if cx else 1.0)
        # row `cancel`: R (9, 5) = (9, 4); entry (9, 50): a - a; entry (9, 51): b - b (1 + 2^-40)
        r1[R1.find(9, 5)] = r1[R1.find(9, 4)]
        a1[A1.find(5, 250)] = -a1[A1.find(4, 250)]
        a1[A1.find(5, 251)] = -a1[A1.find(4, 251)] * (1.0 + 2.0 ** -40)
    rd = rdtype(vt)
    out = dict(R=[r1.astype(rd), r2.astype(rd)], P=[p1.astype(rd), p2.astype(rd)], A=a1.astype(np.dtype(vt)))
    if family == "exact":         # the level-2 sums fit the value type: multiples of 2^-3 below 2^24 (single) - level 3 is asserted on the host
        ref = reference(H["T"][0], out["R"][0], out["A"], out["P"][0])
        assert max(np.abs(ref[0]).max(), np.abs(ref[1]).max()) < 2.0 ** 18
    _VALUES[key] = out
    return out


def initial_coarse(vt, level, seed=3):
    """Values the coarse operators hold at upload (replaced by NaN before every refresh)."""
    C = hierarchy()["C"][level - 2]
    rng = np.random.default_rng([11, level, seed])
    v = rng.standard_normal(C.nnz) + (1j * rng.standard_normal(C.nnz) if vt != "float64" else 0.0)
    return v.astype(np.dtype(vt))


def digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()
