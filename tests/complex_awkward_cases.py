"""TEST INFRASTRUCTURE ONLY.  The awkward-row cases of the complex cycle (tests/test_complex_awkward_host.py, _gpu.py): an operator
whose row blocks reach every edge path of cx_csr_stream_spmv / cx_csr_stream_spmm (mg_complex.hpp), two two-level hierarchies around
it, long-double references and the derived bounds.  numpy / scipy only: imports no device code of the package.

Operator ``awkward6007`` (n = 6007, complex CSR, sorted columns, randn + i randn values, seed 3): base row lengths integers(0, 12)
with 40 random rows emptied; rows 100..103 of 700, 650, 900, 400 entries; row 2000 of 3000; row 2500 of exactly 1024 (the largest row
that still takes the chunk path); row 2501 of 1025 (the smallest that takes the one-long-row branch); rows 3000..3599 of
integers(0, 3) entries with rows 3100..3399 empty; the last row of 900.  ``row_blocks`` restates the partition rule of cx_upload
(consecutive rows, <= MAXROWS = 256 rows and <= CX_CHUNK = 1024 non-zeros, a longer row alone); ``block_classes`` names the blocks.

Hierarchy ``full``: R[i // 7, i] = w_i, P[i, i // 7] = v_i (w, v uniform in [0.5, 1.5]: every fine row is read by R and written by P,
nc = 859), Ac = (4 + i) I + 0.1 sprandom(density 0.05), d = 0.02 (randn + i randn), Jac, V-cycle.  Hierarchy ``sweeps``: the same with
every stored value of P set to 0.0 on the same pattern - the coarse correction adds exact zeros, so a cycle is exactly a chain of
sweeps S(x) = x + d.*(b - A x): S^(pre+post-1)(d.*b) from zero, S^(pre+post)(x0) from an iterate.  The single variants round every
input to complex64 / float32 once; all references are computed from the rounded data.

References are formed in np.clongdouble (64-bit significand, asserted): CSR products by np.add.reduceat, the coarsest solve by
param.LU with three steps of iterative refinement on a long-double residual.

The sweep bound is derived, not measured.  u = 2^-53 (2^-24 in single), u_c = 2 sqrt(2) u covers a complex multiply,
gamma(m) = m u_c / (1 - m u_c), k_i the length of row i.  From zero M = |d||b|, E = gamma(1) M; from an iterate M = |x0|, E = 0; each
sweep M' = M + |d|(|b| + |A| M), E' = gamma(k + 3) M' + E + |d|(|A| E).  Every row must satisfy |got - ref| <= E (a row whose bound
is 0 must be exact; NaN fails).  The norm bound: |got - ref| <= ||E_r||_2 + gamma(N + 4) ref with E_r = gamma(k + 1)(|b| + |A||x|)
row by row in the working precision (0 for the norm of b) and N summed terms in double, in any order.

Measured (recorded from the tests' own output; a bound never comes from these).
Host: 40 row blocks - 3 of 256 rows (one without an entry), 2 long rows, 1 row of exactly 1024 entries, 26 multi-row blocks of >= 1000
entries, the last block a single row.  The plain numpy cycle on ``sweeps``: worst row 0.157 of its bound in double and in single
(allowed 0.25), median E/|x| 2.8e-15 to 2.4e-14 in double, 1.5e-6 to 1.3e-5 in single, max |x| below 40.  ``full``: the complex128
oracle is 2.2e-15 from the long-double cycle in the max norm (allowed 1e-14), the complex64 restatement 4.5e-7 in the 2-norm (allowed
3.8e-6).  Mutations of S(d.*b): a 5-entry row scaled by 1 + 1e-13 is 35 times its bound and 2.8e-14 in the max norm; the 3000-entry row
scaled by 1 + 1e-13 is 0.0036 of its bound and cannot leave it (gamma(3003) = 9.4e-13; the row resolves 2.8e-11 relative), the
1025-entry row 0.035 (gamma(1028) = 3.2e-13; 2.9e-12).  ||b - A x||: relative bound 1.3e-11, numpy's norm uses 1.1e-5 of it.
MI355X, worst row of ``sweeps`` as a share of its bound, the same on both row-pointer widths: vector CF64 0.157 / 0.104 at (1, 1) from
zero / from the iterate, 0.076 / 0.104 at (2, 2); vector CF32 0.157 / 0.108 and 0.078 / 0.107; blocks CF64 at (2, 2), k = 1 .. 16: 0.076
to 0.088 from zero, 0.104 to 0.110 from the iterate; blocks CF32 from zero 0.078 to 0.088.  ``full``: CF64 vector and blocks at most
4.0e-15 from the oracles (allowed 1e-12); CF32 vector 8.5e-8 / 3.3e-7 from the double cycle where the restatement is 1.0e-7 / 3.0e-7,
CF32 blocks at most 1.3e-7 per column (allowed 3.8e-6).  resvec: at most 3.3e-5 of the norm bound (relative bounds 1.9e-12 to 4.2e-11
in double, 6e-3 for a single residual).
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

LD = np.longdouble
CLD = np.clongdouble
assert np.finfo(LD).nmant >= 63, "the reference needs an 80-bit (or wider) long double"

MAXROWS, CX_CHUNK = 256, 1024            # mg_kernels.hpp / mg_complex.hpp
N, NC = 6007, 859
U64, U32 = 2.0 ** -53, 2.0 ** -24
KS = (1, 2, 3, 5, 8, 16)                 # every lane-group width of the block kernel, idle lanes (3, 5) and the cap
SWEEPS_HOST = ((1, 1), (2, 1), (3, 2))


def unit(single):
    return U32 if single else U64


def gamma(m, u):
    """m u_c / (1 - m u_c) with u_c = 2 sqrt(2) u."""
    uc = 2.0 * np.sqrt(2.0) * u
    m = np.asarray(m, dtype=np.float64)
    return m * uc / (1.0 - m * uc)


# ---- the operator and its row blocks -----------------------------------------------------------------------------------------------
_cache = {}


def awkward6007():
    """The operator (complex128 CSR); built once and shared - nothing in it may be modified."""
    if "A" not in _cache:
        n = N
        rng = np.random.default_rng(3)
        lens = rng.integers(0, 12, n)
        lens[rng.choice(n, 40, replace=False)] = 0
        lens[100:104] = [700, 650, 900, 400]
        lens[2000] = 3000
        lens[2500] = CX_CHUNK
        lens[2501] = CX_CHUNK + 1
        lens[3000:3600] = rng.integers(0, 3, 600)
        lens[3100:3400] = 0
        lens[n - 1] = 900
        rows, cols = [], []
        for i, k in enumerate(lens):
            c = np.sort(rng.choice(n, int(k), replace=False))
            rows.append(np.full(len(c), i))
            cols.append(c)
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        vals = rng.standard_normal(len(rows)) + 1j * rng.standard_normal(len(rows))
        A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
        A.sort_indices()
        assert np.array_equal(np.diff(A.indptr), lens)
        _cache["A"] = A
    return _cache["A"]


def row_blocks(indptr):
    """The partition of cx_upload (mg_complex.inc): blk[i] .. blk[i + 1] are the rows of block i."""
    n = len(indptr) - 1
    blk, r = [0], 0
    while r < n:
        e = r + 1
        while e < n and (e - r) < MAXROWS and indptr[e + 1] - indptr[r] <= CX_CHUNK:
            e += 1
        blk.append(e)
        r = e
    return np.array(blk)


def block_classes(indptr):
    """The blocks of each edge class, by block index."""
    blk = row_blocks(indptr)
    rows = np.diff(blk)
    nnz = indptr[blk[1:]] - indptr[blk[:-1]]
    ids = lambda m: [int(i) for i in np.flatnonzero(m)]
    return dict(nblocks=len(rows),
                full_empty=ids((rows == MAXROWS) & (nnz == 0)),
                full=ids((rows == MAXROWS) & (nnz > 0)),
                exact_chunk=ids((rows == 1) & (nnz == CX_CHUNK)),
                long_row=ids((rows == 1) & (nnz > CX_CHUNK)),
                nearly_full=ids((rows > 1) & (nnz >= 1000)),
                last_single=bool(rows[-1] == 1))


# ---- long-double CSR products ------------------------------------------------------------------------------------------------------
class LdCsr:
    """M x in long double for a CSR matrix M (complex or real) and a vector or a block of columns x; empty rows give 0."""

    def __init__(self, M):
        self.shape = M.shape
        self.indices = M.indices
        self.data = M.data.astype(CLD if np.iscomplexobj(M.data) else LD)
        self.len = np.diff(M.indptr).astype(np.int64)
        self.nz = self.len > 0
        self.starts = M.indptr[:-1][self.nz]         # (reduceat over the starts of the non-empty rows: an empty row adds nothing)

    def dot(self, x):
        x = np.asarray(x, dtype=CLD)
        data = self.data if x.ndim == 1 else self.data[:, None]
        prod = data * x[self.indices]
        out = np.zeros((self.shape[0],) + x.shape[1:], dtype=CLD)
        if prod.shape[0]:
            out[self.nz] = np.add.reduceat(prod, self.starts, axis=0)
        return out


def _abs_csr(M):
    return sp.csr_matrix((np.abs(M.data.astype(np.complex128)), M.indices, M.indptr), shape=M.shape)


# ---- the hierarchies ---------------------------------------------------------------------------------------------------------------
class Hierarchy:
    """``full`` or ``sweeps`` in double or single: the operators in the working precision (what a param holds), their long-double
    forms and |A|.  Shared - nothing in it may be modified."""

    def __init__(self, kind, single):
        assert kind in ("full", "sweeps")
        self.kind, self.single = kind, bool(single)
        self.cdtype = np.complex64 if single else np.complex128
        rdtype = np.float32 if single else np.float64
        A = awkward6007()
        n, nc = N, NC
        rng = np.random.default_rng(17)
        i = np.arange(n)
        w, v = rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, n)
        assert (n - 1) // 7 == nc - 1
        R = sp.csr_matrix((w, (i // 7, i)), shape=(nc, n))
        P = sp.csr_matrix((v, (i, i // 7)), shape=(n, nc))
        if kind == "sweeps":
            P.data[:] = 0.0                          # stored zeros on the same pattern: uploaded as they are
        Ac = (sp.identity(nc) * (4.0 + 1j) + 0.1 * sp.random(nc, nc, density=0.05, random_state=19)).tocsr().astype(np.complex128)
        d = 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        for M in (R, P, Ac):
            M.sort_indices()
        assert P.nnz == n and R.nnz == n             # every fine row is read by R and written by P
        self.A, self.Ac = A.astype(self.cdtype), Ac.astype(self.cdtype)
        self.P, self.R = P.astype(rdtype), R.astype(rdtype)
        assert self.P.nnz == n
        self.d = d.astype(self.cdtype)
        self.LU = spla.splu(sp.csc_matrix(self.Ac.astype(np.complex128)))
        self.lA, self.lAc, self.lP, self.lR = LdCsr(self.A), LdCsr(self.Ac), LdCsr(self.P), LdCsr(self.R)
        self.ld = self.d.astype(CLD)
        self.absA = _abs_csr(self.A)
        self.absd = np.abs(self.d.astype(np.complex128))
        self.rowlen = np.diff(self.A.indptr).astype(np.int64)

    def param(self, mg, pre, post):
        """A two-level param around the hierarchy, built by hand as tests/test_complex_gpu.py's _manual_param builds its own."""
        kw = {"singlePrecision": True} if self.single else {}
        p = mg.getMGparam(np.complex128, np.int64, 2, 8, 1, 0.0, "Jac", 0.8, pre, post, "V", "NoMUMPS", 0.5, 0.0, **kw)
        p.As, p.Ps, p.Rs = [self.A, self.Ac], [self.P], [self.R]
        p.relaxPrecs = [self.d]
        p.LU = self.LU
        p.nrhs = 1
        return p


def hierarchy(kind, single):
    key = ("H", kind, bool(single))
    if key not in _cache:
        _cache[key] = Hierarchy(kind, single)
    return _cache[key]


def set_sweeps(p, pre, post):
    p.relaxPre = lambda level, _k=int(pre): _k
    p.relaxPost = lambda level, _k=int(post): _k
    return p


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def vector(seed, single, n=N):
    """randn + i randn, rounded once to the working precision."""
    rng = np.random.default_rng(1000 + seed)
    v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return v.astype(np.complex64 if single else np.complex128)


def zero_column(k):
    """The all-zero interior column of a block of k columns (None: k <= 2 has no interior)."""
    return 1 if k >= 3 else None


def block(seed, single, k):
    """(n, k) complex128, C order: column j is column 0 shifted by 13 j rows and scaled by 2^(3 j - 20) (exact, in single too), one
    interior column all zero."""
    c0 = vector(seed, single).astype(np.complex128)
    B = np.stack([np.roll(c0, 13 * j) * 2.0 ** (3 * j - 20) for j in range(k)], axis=1)
    if zero_column(k) is not None:
        B[:, zero_column(k)] = 0.0
    if single:
        assert np.array_equal(B.astype(np.complex64).astype(np.complex128), B)
    return np.ascontiguousarray(B)


# ---- references --------------------------------------------------------------------------------------------------------------------
def _col(v, x):
    return v if x.ndim == 1 else v[:, None]


def ld_sweep(h, b, x):
    return x + _col(h.ld, x) * (b - h.lA.dot(x))


def sweep_count(pre, post, from_zero):
    return max(pre, 1) + max(post, 1) - (1 if from_zero else 0)


def sweep_chain(h, b, x0, pre, post, from_zero):
    """S^(pre+post-1)(d.*b) from zero, S^(pre+post)(x0) from an iterate, in long double; b, x0: vectors or (n, k) blocks."""
    b = np.asarray(b).astype(CLD)
    x = _col(h.ld, b) * b if from_zero else np.asarray(x0).astype(CLD)
    for _ in range(sweep_count(pre, post, from_zero)):
        x = ld_sweep(h, b, x)
    return x


def sweep_bound(h, b, x0, pre, post, from_zero):
    """E of the module docstring for the same chain, row by row (columns of a block separately), in double."""
    u = unit(h.single)
    ab = np.abs(np.asarray(b).astype(np.complex128))
    ad = _col(h.absd, ab)
    if from_zero:
        M = ad * ab
        E = gamma(1, u) * M
    else:
        M = np.abs(np.asarray(x0).astype(np.complex128))
        E = np.zeros_like(M)
    g = _col(gamma(h.rowlen + 3, u), ab)
    for _ in range(sweep_count(pre, post, from_zero)):
        M = M + ad * (ab + h.absA @ M)
        E = g * M + E + ad * (h.absA @ E)
    return E


def coarse_ld(h, bc):
    """Ac \\ bc in long double: the double factors with iterative refinement on a long-double residual (Ac is strongly diagonally
    dominant: each step gains ~15 digits)."""
    solve = lambda r: h.LU.solve(np.asfortranarray(r.astype(np.complex128))).astype(CLD)
    x = solve(bc)
    for _ in range(3):
        x = x + solve(bc - h.lAc.dot(x))
    return x


def ld_cycle(h, b, x0, pre, post, from_zero):
    """One V-cycle of the two-level hierarchy in long double (the operation sequence of tests/complex_oracle.py)."""
    b = np.asarray(b).astype(CLD)
    if from_zero:
        x = _col(h.ld, b) * b
        first = max(pre, 1) - 1
    else:
        x = np.asarray(x0).astype(CLD)
        first = max(pre, 1)
    for _ in range(first):
        x = ld_sweep(h, b, x)
    xc = coarse_ld(h, h.lR.dot(b - h.lA.dot(x)))
    x = x + h.lP.dot(xc)
    for _ in range(max(post, 1)):
        x = ld_sweep(h, b, x)
    return x


def check_rows(name, got, ref, E):
    """Every row (and column) within its bound; returns the worst |got - ref| / E over the rows with E > 0."""
    err = np.abs(np.asarray(got).astype(CLD) - ref)
    bad = ~(err <= E)                               # (NaN fails; a bound of 0 asks for the exact value)
    pos = E > 0
    worst = float((err[pos] / E[pos]).max()) if pos.any() else 0.0
    if bad.any():
        idx = tuple(int(t[0]) for t in np.nonzero(bad))
        raise AssertionError(f"{name}: {int(bad.sum())} of {err.size} entries outside the componentwise bound (worst ratio {worst:.3g}); "
                             f"first at {idx}: got {np.asarray(got)[idx]!r}, reference {complex(ref[idx])!r}, bound {float(E[idx])!r}")
    return worst


def within_rows(got, ref, E, margin):
    """The worst ratio as check_rows, for a reference run that must use at most `margin` of every bound."""
    err = np.abs(np.asarray(got).astype(CLD) - ref)
    assert np.all(err <= margin * E), "a plain run in the working precision uses more than its share of the bound"
    pos = E > 0
    return float((err[pos] / E[pos]).max())


# ---- the norms of solveMG ----------------------------------------------------------------------------------------------------------
def norm_ld(v):
    v = np.asarray(v).astype(CLD)
    return float(np.sqrt(np.sum(v.real ** 2 + v.imag ** 2)))


def residual_norm(h, b, x=None):
    """(ref, bound) for the norm of b (x None) or of b - A x, Frobenius over the columns of a block: ref in long double,
    bound = ||E_r||_2 + gamma(N + 4) ref, E_r = gamma(k + 1)(|b| + |A||x|) in the working precision, the sum of N terms in double."""
    b = np.asarray(b)
    if x is None:
        ref, er = norm_ld(b), 0.0
    else:
        x = np.asarray(x)
        ref = norm_ld(b.astype(CLD) - h.lA.dot(x.astype(CLD)))
        ab = np.abs(b.astype(np.complex128))
        Er = _col(gamma(h.rowlen + 1, unit(h.single)), ab) * (ab + h.absA @ np.abs(x.astype(np.complex128)))
        er = float(np.sqrt(np.sum(Er ** 2)))
    return ref, er + float(gamma(b.size + 4, U64)) * ref
