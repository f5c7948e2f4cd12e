"""Shared by tests/test_complex_kcycle_block_host.py and tests/test_complex_kcycle_block_gpu.py: the inputs and oracle runs of the
``blockKcycle`` tests (blocks of right-hand sides on K-cycle / Jac-GMRES complex hierarchies), computed once per process and never
modified.  Imports no device code of the package.

THE ORACLE.  The reference runs FGMRES_relaxation on a block as one long vector of length n*k - "one huge block diagonal system"
(FGMRES.jl:51-53).  So no new algorithm is written here: ``kron_param(p, k)`` builds the param of that system - kron(As[l], I_k),
kron(Ps[l], I_k), kron(Rs[l], I_k), repeat(relaxPrecs[l], k), splu of the new coarsest operator - whose vectors are the flat
row-major blocks [n][k], and the existing, unchanged tests/complex_kcycle_oracle.py (tests/complex_single_kcycle_oracle.py for a
ComplexF32 hierarchy) runs on it.  One H, one xi, one t and one break test per relaxation for the whole block follow by themselves.

Column c of a block is 10^(c mod 3) * complex_rhs(n, 9 + c): columns of different scale, so that the coupling through the one t shows.
The operators of the relaxation tests are those of tests/test_complex_kcycle_gpu.py (generators copied), with |d| ~ 0.1."""
import copy

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import complex_kcycle_oracle as korc
from complex_cases import complex_rhs, helmholtz

C128 = np.complex128
EPS = np.finfo(float).eps
PROBLEMS = {"3lev": ([16, 16, 16], 0.5, 3), "4lev": ([16, 16, 16], 0.25, 4)}
SCHEDULES = [("Jac-GMRES", "V", 2, 2), ("Jac-GMRES", "K", 2, 1), ("Jac", "K", 2, 1), ("SPAI", "K", 2, 1), ("Jac-GMRES", "K", 1, 1)]
KS = (3, 16)
BREAK_SCALE = 1e-11          # every relaxation of the two cycles breaks after one direction, every rn a factor >= 110 below 1e-5
                             # (at 1e-9 the clearance is only 1.1 to 2.6: not a scale to test at)


def case_id(v):
    return "-".join(map(str, v)) if isinstance(v, tuple) else str(v)


# ---- the Kronecker param ----------------------------------------------------------------------------------------------------------------
def _kron(M, k):
    K = sp.kron(M, sp.identity(k, dtype=M.dtype, format="csr"), format="csr").astype(M.dtype)
    K.sort_indices()
    return K


def kron_param(p, k, lu=None):
    """The param of the block-diagonal system of k copies of p's hierarchy, interleaved: its vectors are flat row-major blocks [n][k].
    ``lu``: a coarsest solve to use instead of splu of the new coarsest operator (an oracle's solver object)."""
    q = copy.copy(p)
    q.device = None
    q.As = [_kron(A, k) for A in p.As]
    q.Ps = [_kron(P, k) for P in p.Ps]
    q.Rs = [_kron(R, k) for R in p.Rs]
    q.relaxPrecs = [np.repeat(np.asarray(d), k) for d in p.relaxPrecs]
    q.LU = lu if lu is not None else spla.splu(sp.csc_matrix(q.As[-1].astype(C128)), permc_spec="MMD_AT_PLUS_A")
    return q


def flat(B):
    """An n x k block as the long vector of the Kronecker system (row-major)."""
    return np.ascontiguousarray(B).reshape(-1).copy()


def unflat(v, k):
    return np.asfortranarray(v.reshape(-1, k))


def block_rhs(n, k, scale=1.0, seed=9, dtype=C128):
    B = np.stack([scale * 10.0 ** (c % 3) * complex_rhs(n, seed + c) for c in range(k)], axis=1)
    return np.asfortranarray(B.astype(dtype))


# ---- the relaxation cases ---------------------------------------------------------------------------------------------------------------
def _awkward_operator(n, seed):
    """Complex square CSR with empty rows, rows spanning the kernel's 1024-entry chunks and one row longer than a chunk (row 2000:
    3000 entries, the branch in which the lane groups stride over one row)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 12, n)
    lens[rng.choice(n, 40, replace=False)] = 0
    lens[100:104] = [700, 650, 900, 400]
    lens[2000] = 3000
    rows, cols = [], []
    for i, k in enumerate(lens):
        c = np.sort(rng.choice(n, int(k), replace=False))
        rows.append(np.full(len(c), i))
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = rng.standard_normal(len(rows)) + 1j * rng.standard_normal(len(rows))
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    A.sort_indices()
    return A


def _small_operator(n, seed):
    """n <= 256 rows and fewer than 1024 entries: a level of ONE row block."""
    A = (sp.random(n, n, density=3.0 / n, random_state=seed) + 1j * sp.random(n, n, density=3.0 / n, random_state=seed + 1)
         + sp.identity(n) * (3.0 + 1.0j)).tocsr()
    A.sort_indices()
    assert A.nnz < 1024
    return A


def _manual_param(mg, A, nc, seed, single=False):
    """A two-level complex param around an arbitrary A, with |d| ~ 0.1 and ``blockKcycle=True``; ``single``: the ComplexF32 form
    (values rounded to single, ``singleKcycle=True``)."""
    rng = np.random.default_rng(seed)
    n = A.shape[0]
    P = sp.random(n, nc, density=4.0 / nc, random_state=seed, format="csr")
    R = sp.random(nc, n, density=6.0 / n, random_state=seed + 1, format="csr")
    P.sort_indices()
    R.sort_indices()
    Ac = (sp.identity(nc) * (4.0 + 1j) + 0.1 * sp.random(nc, nc, density=0.05, random_state=seed + 2)).tocsr().astype(C128)
    Ac.sort_indices()
    d = 0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    kw = dict(singlePrecision=True, singleKcycle=True) if single else {}
    p = mg.getMGparam(C128, np.int64, 2, 8, 4, 1e-10, "Jac", 0.8, 1, 1, "V", blockKcycle=True, **kw)
    if single:
        A, Ac, d = A.astype(np.complex64), Ac.astype(np.complex64), d.astype(np.complex64)
        P, R = P.astype(np.float32), R.astype(np.float32)
    p.As, p.Ps, p.Rs = [A, Ac], [P], [R]
    p.relaxPrecs = [d]
    p.LU = spla.splu(sp.csc_matrix(Ac.astype(C128)))
    p.nrhs = 1
    return p


_OPS = {"awkward5000": lambda: (_awkward_operator(5000, 3), 700), "oneblock100": lambda: (_small_operator(100, 5), 20)}
_relax_params = {}


def relax_param(mg, name, single=False):
    if (name, single) not in _relax_params:
        A, nc = _OPS[name]()
        _relax_params[(name, single)] = _manual_param(mg, A, nc, 7, single)
    return _relax_params[(name, single)]


def relax_block(n, k, seed=31, scale=1.0):
    """(R0, X0): n x k blocks of O(1) columns (column c: complex_rhs(n, seed + 2 c) and complex_rhs(n, seed + 2 c + 1))."""
    R0 = np.stack([scale * complex_rhs(n, seed + 2 * c) for c in range(k)], axis=1)
    X0 = np.stack([complex_rhs(n, seed + 2 * c + 1) for c in range(k)], axis=1)
    return np.asfortranarray(R0), np.asfortranarray(X0)


def relax_oracle(A, d, R0, X0, inner):
    """FGMRES_relaxation of tests/complex_kcycle_oracle.py on the long vector: (X n x k, rnorms)."""
    n, k = R0.shape
    Afun = lambda v: np.ascontiguousarray(A @ v.reshape(n, k)).reshape(-1)
    dd = np.repeat(d, k)
    x, rn = korc.FGMRES_relaxation(Afun, flat(R0), flat(X0), inner, lambda v: dd * v, korc.GMRES_TOL)
    return unflat(x, k), rn


def relax_bases(A, d, R0, inner):
    """numpy's chain Z_1 = d.*R0, AZ_j = A Z_j, Z_{j+1} = d.*AZ_j as (n, k, inner) arrays, H = (AZ)'(AZ) and xi = (AZ)'R0 in Frobenius
    products of the long vectors."""
    n, k = R0.shape
    Z = np.zeros((n, k, inner), dtype=C128)
    AZ = np.zeros((n, k, inner), dtype=C128)
    z = d[:, None] * R0
    for j in range(inner):
        Z[:, :, j] = z
        AZ[:, :, j] = A @ z
        z = d[:, None] * AZ[:, :, j]
    H, xi = gram_of(AZ, R0)
    return Z, AZ, H, xi


def gram_of(AZ, R0):
    """H[i][j] = <AZ_i, AZ_j>_F and xi[j] = <AZ_j, R0>_F of the (n, k, inner) array AZ."""
    W = AZ.reshape(-1, AZ.shape[2])
    return W.conj().T @ W, W.conj().T @ R0.reshape(-1)


# ---- the cycle cases --------------------------------------------------------------------------------------------------------------------
_params, _cycles = {}, {}


def helm_param(mg, prob, sched, maxIter=5, tol=1e-10, damping=0.5, coarse="NoMUMPS", **kw):
    cells, kh, levels = PROBLEMS[prob]
    A, mesh = helmholtz(mg, cells, kh, damping)
    relax, cyc, pre, post = sched
    kw.setdefault("blockKcycle", True)
    p = mg.getMGparam(C128, np.int64, levels, 8, maxIter, tol, relax, 0.8, pre, post, cyc, coarse, 0.5, 0.0, **kw)
    mg.MGsetup(A, mesh, p)
    return p


def cycle_param(mg, prob, sched):
    """The ``blockKcycle`` param of a cycle case, shared by every k and scale: never modified, never uploaded by a test (a test
    builds its own DeviceHierarchy from it)."""
    if (prob, sched) not in _params:
        _params[(prob, sched)] = helm_param(mg, prob, sched)
    return _params[(prob, sched)]


def two_cycles(mg, prob, sched, k, scale):
    """dict(p, B, X1, X2, trace): the block, the Kronecker oracle's iterate after one cycle from zero and after a second from the
    first iterate (n x k, Fortran-ordered), and the trace of both."""
    key = (prob, sched, k, scale)
    if key not in _cycles:
        p = cycle_param(mg, prob, sched)
        q = kron_param(p, k)
        B = block_rhs(p.As[0].shape[0], k, scale)
        trace = []
        b = flat(B)
        x1 = korc.recursiveCycle(q, b, np.zeros_like(b), 1, trace=trace).copy()
        x2 = korc.recursiveCycle(q, b, x1.copy(), 1, trace=trace).copy()
        _cycles[key] = dict(p=p, B=B, X1=unflat(x1, k), X2=unflat(x2, k), trace=trace)
    return _cycles[key]


def columnwise_cycle(p, B):
    """One vector-oracle cycle from zero on every column by itself: what a column-by-column implementation computes."""
    return np.asfortranarray(np.stack([korc.recursiveCycle(p, np.ascontiguousarray(B[:, c]), np.zeros(B.shape[0], dtype=C128), 1).copy()
                                       for c in range(B.shape[1])], axis=1))


def kron_preconditioner(p, k, trace=None):
    """M(V) for n x k blocks: one Kronecker-oracle cycle from zero."""
    q = kron_param(p, k)
    mem = korc._Mem(q)

    def M(V):
        v = flat(np.asarray(V, dtype=C128))
        return unflat(korc.recursiveCycle(q, v, np.zeros_like(v), 1, mem, None, trace).copy(), k)

    return M


# ---- the GMRES coarsest solve under a block K-cycle -------------------------------------------------------------------------------------
class FlatBlockCoarse:
    """The block GMRES coarsest solve (complex_block_coarse_cases.OracleBlockCoarseGmres: blockFGMRES on the n_c x k block, as the
    reference calls it for a block, MGcycle.jl:165-167) behind the Kronecker param's ``LU.solve`` of a flat row-major vector."""

    def __init__(self, inner, k):
        self.inner, self.k = inner, k

    def solve(self, b):
        return np.ascontiguousarray(self.inner.solve(np.asarray(b, dtype=C128).reshape(-1, self.k))).reshape(-1)


GMRES_COARSE = ("3lev", ("Jac", "K", 2, 1), 0.2, 3)      # (problem, schedule, damping, k) of the GMRES-coarse case
_gmres = {}


def gmres_coarse_cycle(mg):
    """dict(p, B, X1, trace, log): one block cycle from zero on a ``blockCoarseGMRES`` + ``blockKcycle`` hierarchy by the Kronecker
    oracle with the block coarsest solve, the K-cycle's trace and the coarsest solve's log."""
    if not _gmres:
        import complex_block_coarse_cases as cbc
        prob, sched, damping, k = GMRES_COARSE
        p = helm_param(mg, prob, sched, damping=damping, coarse="GMRES", blockCoarseGMRES=True)
        orc = cbc.OracleBlockCoarseGmres(p.As[-1], p.LU)
        q = kron_param(p, k, lu=FlatBlockCoarse(orc, k))
        B = block_rhs(p.As[0].shape[0], k)
        trace = []
        b = flat(B)
        x1 = korc.recursiveCycle(q, b, np.zeros_like(b), 1, trace=trace).copy()
        _gmres.update(p=p, B=B, X1=unflat(x1, k), trace=trace, log=orc.log)
    return _gmres
