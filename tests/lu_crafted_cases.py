"""TEST INFRASTRUCTURE ONLY.  Crafted sparse factors for the stand-alone factor applier (mg_lu_*_FP64 / mg_lu_*_CFP64;
tests/test_lu_crafted_host.py, _gpu.py): hand-made L and U in parLU's layout whose rows, levels and trailing blocks reach the edge
paths of sptrsv_lu / sptrsv_sweep, sptrsv_level / sptrsv_tail_rhs / sptrsv_scatter, tri_gather_block / tri_inverse / tri_apply
(mg_kernels.hpp) and their cx_ twins (mg_complex.hpp), long-double references and the derived bounds.  numpy only: imports no device
code of the package.  Nothing is factorised: a case IS its factors, A = P' L U Q' is only assembled to check the reference.

Layout: 1-based Int64 CSR, L's diagonal last in each row, U's first; p, q random 1-based permutations, p != q, neither the identity;
x[q] = U \\ (L \\ b[p]) and, for doTranspose, x[p] = L' \\ (U' \\ b[q]) (' = transpose for real, adjoint for complex factors).  Every
pattern is generated level by level (a row of level l holds one entry of level l - 1 and the others below l) and then relabelled by a
random topological order, so `order` / the slot tables are no identity.  Each diagonal has modulus in [1, 2] and a random sign
(real) or phase (complex); an off-diagonal (i, j) has modulus 0.5 r / max(entries of row i, entries of column j), r in [0.5, 1]:
the off-diagonal moduli of every row AND of every column sum to at most 0.5, so both solve directions are well conditioned and the
running bound does not grow along a chain.  The real and the complex variant share patterns and moduli.

Family ``levels`` (n = 697, no trailing chain): level sizes LEVEL_SIZES - 340 rows without an entry, wide levels of 70 and 100 rows,
levels of 17, 16, 15, 5, 3, 2 and 1 rows (g = 16 / rows changes: 1, 1, 1, 2, 4, 8, 16) - rows of exactly 1, 63, 64, 65, 128, 129 and
300 off-diagonal entries placed in the small levels and the wide one (LONG_ROWS), the rest 1 to 8 (0 in the first level); columns
of exactly 63 .. 300 entries (LONG), so that after the transposition both directions again hold such rows.  U is a second pattern of
the same recipe (another seed, other values), mirrored.  Family ``tail(M)``, M in TAILS (n = 600 + M): the last M rows and columns
of L and U hold a full triangle - a chain of M single-row levels in both factors, before and after transposition; every tail row of L
holds 70 to 140 entries left of the block (one of them in the last level above; the first tail row all 600, as column n - M of U), every row of U above the tail holds column n - M and
16 to 24 further tail columns.  ``choose_tail`` restates the tail-size choice of mg_set_coarse_lu_FP64_INT64 / cxlu_upload: with
MG_LU_DENSE_TAIL_MIN = MAX = M it must pick M for all four factor sets.  Family ``exact``: the ``levels`` recipe cut to 6 levels
(590, 70, 17, 5, 2, 1) with at most 3 off-diagonals, and tails of 33 and 65 whose block is the identity plus a sub- / super-diagonal;
all values from {+-1, +-i} (real: +-1), right-hand sides integers in [-3, 3]: the solution is a (Gaussian) integer, computed with
Python integers, every partial sum on the device is an integer far below 2^53 - nothing rounds, the result must be bit-equal.

Reference: row-wise substitution in np.longdouble / np.clongdouble (64-bit significand, asserted).

Bound (derived; never measured from a device).  u = 2^-53, u_c = 2 sqrt(2) u for complex and u for real factors,
gamma(m) = m u_c / (1 - m u_c).  A substituted row i with k_i off-diagonals t_ij, diagonal t_ii and right-hand side rhs_i (b[p] for L,
L's result for U, then with its own bound E_rhs):
    E_i = ( gamma(k_i + 3) (|rhs_i| + sum_j |t_ij| |y_j|) + E_rhs_i + sum_j |t_ij| E_j ) / |t_ii| + gamma(2) |y_i|
k_i products (each within u_c), at most k_i - 1 additions in ANY order (lanes, parts, a butterfly: the bound does not ask) and one
subtraction stay within gamma(k_i + 1) of the numerator's terms; the division, which the device forms as a conj(d) / |d|^2, is within
(3 + 2 sqrt 2) u = 2.07 u_c of the quotient, which gamma(2) |y_i| and the two u_c left on the numerator cover.  For real factors the
same counts hold with u.  The trailing block T (M x M) is applied through a
computed inverse X^, so its rows are not backward stable one by one.  With t the block's right-hand side (b[p] minus the entries left
of the block for L - E_t as a substituted numerator with the count of those entries; U takes L's tail as it is):
    E_tail = |T^-1| gamma(c M) |T| |T^-1| |t|  +  gamma(M + 2) |T^-1| |t|  +  |T^-1| E_t
The first term: each column of X^ is a blocked substitution of T x = e_j, so (T + dT) x^ = e_j with |dT| <= gamma(c M) |T|.  c M counts
what one term of a row passes through in tri_inverse / cx_tri_inverse: its product, at most M - 1 additions (the panel product and the
substitution inside the diagonal block, in any order), the subtraction from the identity and the division (< 3 u_c): c M = M + 4, that
is c = 1 + 4 / M.  |T^-1| comes from long-double substitution on the identity.  All bounds are first order in u; the neglected terms
are below 1e-12 of a bound (gamma(M + 4) | |T^-1| |T| | < 1e-12 for these factors).
Condition: every entry of every column |got - ref| <= E, NaN fails; family ``exact``: equal bit for bit.

Measured (recorded from the tests' own output; a bound never comes from these).
Host (tests/test_lu_crafted_host.py).  The reference against the assembled matrix: at most 6.3 long-double ulps of |L||U||x| + |b|
(allowed 16).  Worst entry of the plain numpy double model as a share of its bound (allowed 0.25), plain / transposed: ``levels``
complex 0.142 / 0.111, real 0.163 / 0.188, the same in the lane-strided and in the g-split order; ``tail(1)`` complex 0.140 / 0.141,
real 0.212 / 0.197; ``tail(M)``, M >= 31: complex 0.034 to 0.107, real 0.055 to 0.172.  The trailing block alone (E_t = 0): M = 1
complex 0.064, real 0.169 (one division against gamma(5) + gamma(3)); M >= 31 complex 0.005 to 0.018, real 0.014 to 0.056.  Median
E / |x|: 5.7e-15 to 2.3e-14 complex, 2.1e-15 to 9.1e-15 real.  One thing wrong: the 65-entry row without its last entry 3.6e11
(complex) and 3.2e12 (real) times the bound; one entry of a short row scaled by 1 + 2^-40 103 and 461 times (and below 1e-12 of
max|x|); b[q] for b[p] above 1e6 times; the tail product with ld = M at M = 33 2.9e13 to 4.8e14 times, tri_apply<false> started at
the next multiple of 64 5.8e12 to 3.9e13 times.
MI355X (tests/test_lu_crafted_gpu.py), worst entry over nrhs 1 .. 9 as a share of its bound, plain / transposed: ``levels`` complex
0.112 / 0.098 and real 0.163 / 0.188, the same figures from the single workgroup and from the chip-wide form; ``tail(1)`` complex
0.124 / 0.127, real 0.212 / 0.197; ``tail(M)``, M >= 31: complex 0.032 to 0.111, real 0.055 to 0.172.  mg_lu_form confirmed every M
in both directions for both value types; every ``exact`` case came out bit-equal; the device entry gave the host entry's bits.
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
assert np.finfo(LD).nmant >= 63, "the reference needs an 80-bit (or wider) long double"

U64 = 2.0 ** -53
NW = 16                                     # wavefronts of sptrsv_lu's one workgroup (mg_kernels.hpp)
NRHS = (1, 2, 3, 4, 5, 7, 8, 9)             # a group of three, a full group, the boundary, two groups and one more
KMAX = max(NRHS)
TAILS = (1, 31, 32, 33, 63, 64, 65, 129)
EXACT_TAILS = (33, 65)
LONG = (300, 129, 128, 65, 64, 63)          # exact entry counts: of rows and, for the transposed direction, of columns
LEVEL_SIZES = (340, 70, 17, 16, 15, 5, 3, 2, 1, 100, 60, 30, 20, 12, 6)
LONG_ROWS = {1: (63, 64, 65, 128), 2: (65,), 3: (64,), 4: (63,), 5: (129, 64), 6: (128, 65, 1), 7: (300, 129), 8: (300,), 9: (65, 129)}
EXACT_SIZES = (590, 70, 17, 5, 2, 1)
TAIL_TOP = (360, 120, 70, 35, 15)           # the 600 rows above a trailing block
N_TOP = sum(TAIL_TOP)


def gamma(m, cx):
    """m u_c / (1 - m u_c), u_c = 2 sqrt(2) u for complex factors and u for real ones."""
    uc = (2.0 * np.sqrt(2.0) if cx else 1.0) * U64
    m = np.asarray(m, dtype=np.float64)
    return m * uc / (1.0 - m * uc)


def split(cnt):
    """g of sptrsv_sweep: the wavefronts that share one row of a level of cnt rows."""
    g = 1
    while g * 2 * cnt <= NW:
        g *= 2
    return g


# ---- triangular factors ------------------------------------------------------------------------------------------------------------
class Tri:
    """A triangular factor: 0-based CSR of the off-diagonals (columns ascending in every row) and the diagonal apart."""

    def __init__(self, lower, ptr, col, val, diag):
        self.lower, self.n = bool(lower), len(diag)
        self.ptr, self.col, self.val, self.diag = ptr, col, val, diag
        self.len = np.diff(ptr)

    def row(self, i):
        s = slice(self.ptr[i], self.ptr[i + 1])
        return self.col[s], self.val[s]

    def adjoint(self):
        """Conjugate transpose (the transpose of a real factor), columns again ascending."""
        order = np.argsort(self.col, kind="stable")
        rows = np.repeat(np.arange(self.n), self.len)
        cnt = np.bincount(self.col, minlength=self.n)
        ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        return Tri(not self.lower, ptr, rows[order].astype(np.int64), np.conj(self.val[order]), np.conj(self.diag))

    def parlu(self):
        """(ptr, col, val) in parLU's layout: 1-based Int64, L's diagonal last in its row, U's first."""
        n, i = self.n, np.arange(self.n)
        ptr = self.ptr + np.arange(n + 1)
        rows = np.repeat(i, self.len)
        k = np.arange(len(self.col)) + rows + (0 if self.lower else 1)
        d = (ptr[1:] - 1) if self.lower else ptr[:-1]
        col = np.empty(ptr[-1], dtype=np.int64)
        val = np.empty(ptr[-1], dtype=self.val.dtype)
        col[k], val[k], col[d], val[d] = self.col, self.val, i, self.diag
        return np.ascontiguousarray(ptr + 1, dtype=np.int64), col + 1, np.ascontiguousarray(val)

    def dense(self, r0=0):
        """Rows and columns r0.. as a dense long-double block."""
        m = self.n - r0
        T = np.zeros((m, m), dtype=CLD if np.iscomplexobj(self.val) else LD)
        for i in range(m):
            c, v = self.row(r0 + i)
            T[i, c[c >= r0] - r0] = v[c >= r0]
            T[i, i] = self.diag[r0 + i]
        return T


def _tri(lower, rows, vals, diag):
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.concatenate(rows).astype(np.int64) if ptr[-1] else np.zeros(0, dtype=np.int64)
    return Tri(lower, ptr, col, np.concatenate(vals) if ptr[-1] else np.zeros(0, dtype=diag.dtype), diag)


def lu_levels(T, M=0):
    """The level of every row of [0, n - M): lu_levels of mg_formats.inc restated (for U the trailing M columns impose nothing)."""
    na = T.n - M
    lvl = np.zeros(na, dtype=np.int64)
    for i in (range(na) if T.lower else range(na - 1, -1, -1)):
        c = T.row(i)[0]
        c = c[c < na]
        if len(c):
            lvl[i] = lvl[c].max() + 1
    return lvl


def level_sizes(T, M=0):
    lvl = lu_levels(T, M)
    return np.bincount(lvl) if len(lvl) else np.zeros(0, dtype=np.int64)


def choose_tail(L, U, tmin, tmax, cx):
    """The order of the trailing block as mg_set_coarse_lu_FP64_INT64 / cxlu_upload choose it."""
    cap = min(tmax, L.n)
    best, M, cand = 0.0, 0, 0
    while cand <= cap:
        est = 8e-6 * (len(level_sizes(L, cand)) + len(level_sizes(U, cand))) + 2.0 * (8.0 if cx else 4.0) * cand * cand / 4e12
        if cand == 0 or est < best:
            best, M = est, cand
        cand = max(tmin, 1) if cand == 0 else cand * 2
    return M


# ---- patterns ----------------------------------------------------------------------------------------------------------------------
def _relabel(rows, rng):
    """A random topological relabelling: the pattern stays lower triangular, its levels stay what they are."""
    n = len(rows)
    key = np.zeros(n)
    for i in range(n):
        key[i] = key[rows[i]].max() + rng.uniform(0.01, 1.0) if len(rows[i]) else rng.uniform(0.0, 6.0)
    new = np.empty(n, dtype=np.int64)
    new[np.argsort(key, kind="stable")] = np.arange(n)
    out = [None] * n
    for i in range(n):
        out[new[i]] = np.sort(new[rows[i]]) if len(rows[i]) else np.zeros(0, dtype=np.int64)
    return out


def _gen_lower(sizes, long_rows, long_cols, kmax, rng):
    """Lower-triangular off-diagonal pattern with the given level sizes; long_rows {level: entry counts}, long_cols: entry counts
    of columns (rows of the first level that only the short rows reference)."""
    n = int(sum(sizes))
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    level_of = np.repeat(np.arange(len(sizes)), sizes)
    special = np.zeros(n, dtype=bool)
    scols = rng.choice(sizes[0], len(long_cols), replace=False)
    special[scols] = True
    want = {}
    for l, counts in long_rows.items():
        for j, k in enumerate(counts):
            want[int(start[l] + j)] = int(k)
    rest = [i for i in range(int(start[1]), n) if i not in want]
    forced = {i: [] for i in rest}
    for c, m in zip(scols, long_cols):
        cand = [i for i in rest if len(forced[i]) < 5]
        for i in rng.choice(cand, m, replace=False):
            forced[int(i)].append(int(c))
    rows = [np.zeros(0, dtype=np.int64) for _ in range(n)]
    idx = np.arange(n)
    for i in range(int(start[1]), n):
        l = level_of[i]
        prev = idx[start[l - 1]:start[l]]
        prev = prev[~special[prev]]
        below = idx[:start[l]]
        below = below[~special[below]]
        f = forced.get(i, [])
        k = want[i] if i in want else max(int(rng.integers(1, kmax + 1)), len(f) + 1)
        first = int(rng.choice(prev))
        others = rng.choice(below[below != first], k - 1 - len(f), replace=False)
        rows[i] = np.sort(np.concatenate([[first], others, f]).astype(np.int64))
    return _relabel(rows, rng)


def _mirror(rows):
    n = len(rows)
    return [np.sort(n - 1 - rows[n - 1 - i]) for i in range(n)]


def _values(rows, rng, unit):
    """(moduli and phases) -> complex values per row and the diagonal; `unit`: every value from {1, -1, i, -i}."""
    n = len(rows)
    cnt_r = np.array([len(r) for r in rows])
    allc = np.concatenate(rows) if cnt_r.sum() else np.zeros(0, dtype=np.int64)
    cnt_c = np.bincount(allc, minlength=n)
    vals = []
    for i, r in enumerate(rows):
        k4, th, rr = rng.integers(0, 4, len(r)), rng.uniform(0, 2 * np.pi, len(r)), rng.uniform(0.5, 1.0, len(r))
        vals.append((1j ** k4).astype(np.complex128) if unit else 0.5 * rr / np.maximum(cnt_r[i], cnt_c[r]) * np.exp(1j * th))
    k4, th, rr = rng.integers(0, 4, n), rng.uniform(0, 2 * np.pi, n), rng.uniform(1.0, 2.0, n)
    diag = (1j ** k4).astype(np.complex128) if unit else rr * np.exp(1j * th)
    return vals, diag


def _real(v):
    """The real variant of a complex value: the same modulus, the sign of its real part (of the imaginary part where that is 0)."""
    s = np.where(v.real != 0, np.sign(v.real), np.sign(v.imag))
    return np.abs(v) * s


# ---- cases -------------------------------------------------------------------------------------------------------------------------
class Case:
    """One set of factors: L, U (Tri), 0-based p, q, the order M of the trailing block the chip-wide form is to take (0: none)."""

    def __init__(self, name, cx, L, U, p, q, M, exact):
        self.name, self.cx, self.L, self.U, self.p, self.q, self.M, self.exact = name, cx, L, U, p, q, M, exact
        self.n = L.n
        self.dtype = np.complex128 if cx else np.float64
        self._adj = None

    def factors(self, t):
        """(lower, upper, p_in, p_out) of the solve x[p_out] = upper \\ (lower \\ b[p_in]) for doTranspose = t."""
        if not t:
            return self.L, self.U, self.p, self.q
        if self._adj is None:
            self._adj = (self.U.adjoint(), self.L.adjoint())
        return self._adj[0], self._adj[1], self.q, self.p

    def abi(self):
        """The arrays of mg_lu_create_*_INT64."""
        Lp, Lc, Lv = self.L.parlu()
        Up, Uc, Uv = self.U.parlu()
        return dict(Lp=Lp, Lc=Lc, Lv=Lv, Up=Up, Uc=Uc, Uv=Uv, p=np.ascontiguousarray(self.p + 1), q=np.ascontiguousarray(self.q + 1))

    def rhs(self):
        """(n, KMAX) right-hand sides; the first k columns serve nrhs = k."""
        rng = np.random.default_rng(4242 + self.n)
        if self.exact:
            B = rng.integers(-3, 4, (self.n, KMAX)) + 1j * rng.integers(-3, 4, (self.n, KMAX))
        else:
            B = rng.standard_normal((self.n, KMAX)) + 1j * rng.standard_normal((self.n, KMAX))
        return np.ascontiguousarray(B.astype(np.complex128) if self.cx else B.real.astype(np.float64))


_cache = {}


def _perms(n, rng):
    p, q = rng.permutation(n).astype(np.int64), rng.permutation(n).astype(np.int64)
    ident = np.arange(n)
    assert not np.array_equal(p, q) and not np.array_equal(p, ident) and not np.array_equal(q, ident)
    return p, q


def _finish(name, Lrows, Urows, M, exact, rng):
    Lv, Ld = _values(Lrows, rng, exact)
    Uv, Ud = _values(Urows, rng, exact)
    if exact and M:                                # the block is the identity plus one side diagonal
        Ld[-M:], Ud[-M:] = 1.0, 1.0
    p, q = _perms(len(Lrows), rng)
    for cx in (True, False):
        conv = (lambda v: v) if cx else (lambda v: np.ascontiguousarray(_real(v)))
        L = _tri(True, Lrows, [conv(v) for v in Lv], conv(Ld))
        U = _tri(False, Urows, [conv(v) for v in Uv], conv(Ud))
        _cache[(name, cx)] = Case(name, cx, L, U, p, q, M, exact)


def _build_levels(name, sizes, long_rows, long_cols, kmax, exact, seed):
    rng = np.random.default_rng(seed)
    Lrows = _gen_lower(sizes, long_rows, long_cols, kmax, rng)
    Urows = _mirror(_gen_lower(sizes, long_rows, long_cols, kmax, rng))
    _finish(name, Lrows, Urows, 0, exact, rng)


def _build_tail(name, M, exact, seed):
    rng = np.random.default_rng(seed)
    n0, n = N_TOP, N_TOP + M
    kmax = 2 if exact else 8
    Ltop = _gen_lower(TAIL_TOP, {}, (), kmax, rng)
    Utop = _mirror(_gen_lower(TAIL_TOP, {}, (), kmax, rng))
    lvl = np.zeros(n0, dtype=np.int64)
    for i in range(n0):
        lvl[i] = lvl[Ltop[i]].max() + 1 if len(Ltop[i]) else 0
    last = np.flatnonzero(lvl == lvl.max())
    Lrows, Urows = list(Ltop), []
    for i in range(M):                             # the tail of L: entries left of the block, then the block's row
        k = 2 if exact else (n0 if i == 0 else 140 if i == M // 2 else int(rng.integers(70, 91)))
        first = int(rng.choice(last))
        left = np.concatenate([[first], rng.choice(np.delete(np.arange(n0), first), k - 1, replace=False)])
        blk = (np.arange(n0 + i - 1, n0 + i) if i else np.zeros(0)) if exact else np.arange(n0, n0 + i)
        Lrows.append(np.concatenate([np.sort(left), blk]).astype(np.int64))
    for i in range(n0):                            # rows of U above the tail: column n0 and further tail columns
        k = 0 if exact else min(M - 1, int(rng.integers(16, 25)))
        more = n0 + 1 + rng.choice(M - 1, k, replace=False) if k else np.zeros(0)
        Urows.append(np.concatenate([Utop[i], [n0], np.sort(more)]).astype(np.int64))
    for i in range(M):
        blk = np.arange(n0 + i + 1, min(n0 + i + 2, n)) if exact else np.arange(n0 + i + 1, n)
        Urows.append(blk.astype(np.int64))
    _finish(name, Lrows, Urows, M, exact, rng)


def case(name, cx):
    """``levels``, ``tail33`` .., ``exact_levels``, ``exact_tail33`` ..; built once and shared - nothing in it may be modified."""
    if (name, cx) not in _cache:
        if name == "levels":
            _build_levels(name, LEVEL_SIZES, LONG_ROWS, LONG, 8, False, 71)
        elif name == "exact_levels":
            _build_levels(name, EXACT_SIZES, {}, (), 3, True, 72)
        elif name.startswith("exact_tail"):
            _build_tail(name, int(name[10:]), True, 7300 + int(name[10:]))
        elif name.startswith("tail"):
            _build_tail(name, int(name[4:]), False, 7400 + int(name[4:]))
        else:
            raise KeyError(name)
    return _cache[(name, cx)]


# ---- the reference and its bound ---------------------------------------------------------------------------------------------------
def _sub_rows(T, rows, rhs, Erhs, y, E, cx):
    """Row-wise substitution of the given rows (in dependency order) in long double, E_i of the module docstring beside it."""
    ad = np.abs(T.diag.astype(np.complex128))
    for i in rows:
        c, v = T.row(i)
        av = np.abs(v.astype(np.complex128))[:, None]
        s = (v.astype(y.dtype)[:, None] * y[c]).sum(axis=0)
        y[i] = (rhs[i] - s) / T.diag[i].astype(y.dtype)
        num = np.abs(rhs[i]).astype(np.float64) + (av * np.abs(y[c]).astype(np.float64)).sum(axis=0)
        E[i] = (gamma(len(c) + 3, cx) * num + Erhs[i] + (av * E[c]).sum(axis=0)) / ad[i] + gamma(2, cx) * np.abs(y[i]).astype(np.float64)


def tail_parts(T, n0):
    """(T, T^-1) of the trailing block in long double; the inverse by substitution on the identity."""
    D = T.dense(n0)
    M = D.shape[0]
    X = np.zeros_like(D)
    I = np.eye(M, dtype=D.dtype)
    for i in (range(M) if T.lower else range(M - 1, -1, -1)):
        X[i] = (I[i] - D[i] @ X) / D[i, i]            # (X[i] is still zero here: the sum runs over the rows already known)
    return D, X


def _tail(T, n0, t, Et, y, E, cx):
    """The trailing block applied to t: the reference by substitution, E_tail of the module docstring."""
    D, X = tail_parts(T, n0)
    M = D.shape[0]
    z = np.zeros_like(t)
    for i in (range(M) if T.lower else range(M - 1, -1, -1)):
        z[i] = (t[i] - D[i] @ z) / D[i, i]
    aD, aX, at = np.abs(D).astype(np.float64), np.abs(X).astype(np.float64), np.abs(t).astype(np.float64)
    xt = aX @ at
    y[n0:] = z
    E[n0:] = aX @ (gamma(M + 4, cx) * (aD @ xt)) + gamma(M + 2, cx) * xt + aX @ Et


def reference(c, t, B=None):
    """(X, E): the long-double solution for doTranspose = t and the bound of every entry, for the form the case is made for
    (c.M > 0: the trailing block through its inverse)."""
    key = ("ref", c.name, c.cx, t)
    if B is None and key in _cache:
        return _cache[key]
    lo, up, pin, pout = c.factors(t)
    n, M = c.n, c.M
    n0 = n - M
    wide = CLD if c.cx else LD
    b = (c.rhs() if B is None else B).astype(wide)[pin]
    k = b.shape[1]
    y, E = np.zeros((n, k), dtype=wide), np.zeros((n, k))
    _sub_rows(lo, range(n0), b, np.zeros((n, k)), y, E, c.cx)
    if M:
        tt, Et = np.zeros((M, k), dtype=wide), np.zeros((M, k))
        for i in range(M):                        # t = b[p] - (the entries left of the block) y: a substituted numerator
            cc, v = lo.row(n0 + i)
            v, cc = v[cc < n0], cc[cc < n0]
            av = np.abs(v.astype(np.complex128))[:, None]
            tt[i] = b[n0 + i] - (v.astype(wide)[:, None] * y[cc]).sum(axis=0)
            num = np.abs(b[n0 + i]).astype(np.float64) + (av * np.abs(y[cc]).astype(np.float64)).sum(axis=0)
            Et[i] = gamma(len(cc) + 3, c.cx) * num + (av * E[cc]).sum(axis=0)
        _tail(lo, n0, tt, Et, y, E, c.cx)
    z, F = np.zeros_like(y), np.zeros_like(E)
    if M:
        _tail(up, n0, y[n0:].copy(), E[n0:].copy(), z, F, c.cx)
    _sub_rows(up, range(n0 - 1, -1, -1), y, E, z, F, c.cx)
    X, EX = np.zeros_like(z), np.zeros_like(F)
    X[pout], EX[pout] = z, F
    if B is None:
        _cache[key] = (X, EX)
    return X, EX


def exact_solution(c, t):
    """The solution of an ``exact`` case in Python integers (Gaussian integers as pairs), as an array of the case's dtype."""
    key = ("exact", c.name, c.cx, t)
    if key in _cache:
        return _cache[key]
    lo, up, pin, pout = c.factors(t)
    n = c.n
    gi = lambda z: (int(round(complex(z).real)), int(round(complex(z).imag)))
    mul = lambda a, b: (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])
    B = c.rhs()
    out = np.zeros((n, KMAX), dtype=c.dtype)
    big = 0
    for col in range(KMAX):
        rhs = [gi(B[pin[i], col]) for i in range(n)]
        for T, rows in ((lo, range(n)), (up, range(n - 1, -1, -1))):
            y = [None] * n
            for i in rows:
                cc, v = T.row(i)
                a = rhs[i]
                for j, w in zip(cc, v):
                    m = mul(gi(w), y[j])
                    a = (a[0] - m[0], a[1] - m[1])
                d = gi(T.diag[i])
                assert d[0] * d[0] + d[1] * d[1] == 1
                y[i] = mul(a, (d[0], -d[1]))      # a unit's inverse is its conjugate
            rhs = y
        for i in range(n):
            big = max(big, abs(rhs[i][0]), abs(rhs[i][1]))
            out[pout[i], col] = complex(*rhs[i]) if c.cx else float(rhs[i][0])
            assert c.cx or rhs[i][1] == 0
    assert big < 2 ** 40, "an exact case must stay far below 2^53"
    _cache[key] = out
    return out


def check(name, got, ref, E):
    """Every entry within its bound; returns the worst |got - ref| / E over the entries with E > 0."""
    err = np.abs(np.asarray(got).astype(ref.dtype) - ref).astype(np.float64)
    bad = ~(err <= E)                               # (NaN fails; a bound of 0 asks for the exact value)
    pos = E > 0
    worst = float((err[pos] / E[pos]).max()) if pos.any() else 0.0
    if bad.any():
        idx = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError(f"{name}: {int(bad.sum())} of {err.size} entries outside the componentwise bound (worst ratio {worst:.3g}); "
                             f"first at {idx}: got {np.asarray(got)[idx]!r}, reference {complex(ref[idx])!r}, bound {float(E[idx])!r}")
    return worst


def share(got, ref, E):
    """The worst |got - ref| / E, no assertion (a NaN gives inf)."""
    err = np.abs(np.asarray(got).astype(ref.dtype) - ref).astype(np.float64)
    r = np.where(E > 0, err / np.where(E > 0, E, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.nan_to_num(r, nan=np.inf).max())
