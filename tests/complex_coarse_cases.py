"""TEST INFRASTRUCTURE ONLY.  The GMRES coarsest solve of a complex hierarchy (coarseSolveType = "GMRES"; MGsetup.jl:335-336,
MGcycle.jl:152-164) as the oracles see it, and the operators and hierarchies its tests share.  Imports no device code of the package.

``OracleCoarseGmres`` is an object with ``.solve(b)``: x = 0, then one restart of ``complex_krylov_oracle.fgmres(A_c., b, 10,
tol = 0.01, maxIter = 1, M = d.)``.  Put into ``param.LU`` of a COPY of a param (``oracle_param``), it lets tests/complex_oracle.py and
tests/complex_kcycle_oracle.py run unchanged, and it logs (flag, steps, resvec) of every call.

``clearance(log)``: the break at err <= 0.01 is a discrete decision, so every comparison with the device first asserts ON THE ORACLE'S
LOG ALONE that no logged estimate lies within a factor 1.5 of 0.01 - the smallest over all estimates of max(e / 0.01, 0.01 / e).  If that
fails the input is wrong: change the input, never the factor."""
from __future__ import annotations

import copy

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import complex_krylov_oracle as ck
from complex_cases import complex_rhs, helmholtz

CG_STEPS, CG_TOL = 10, 0.01
MIN_CLEARANCE = 1.5


class OracleCoarseGmres:
    def __init__(self, Ac, d):
        self.A = sp.csr_matrix(Ac, dtype=np.complex128)
        self.d = np.asarray(d, dtype=np.complex128)
        self.log = []

    def solve(self, b):
        b = np.asarray(b, dtype=np.complex128)
        x, flag, steps, resvec = ck.fgmres(lambda v: self.A @ v, b, CG_STEPS, CG_TOL, 1, lambda v: self.d * v, np.zeros_like(b))
        self.log.append((flag, steps, np.array(resvec)))
        return x


def clearance(log):
    c = np.inf
    for _, _, resvec in log:
        for e in resvec:
            c = min(c, max(e / CG_TOL, CG_TOL / e) if e > 0 else np.inf)
    return c


def oracle_param(p):
    """A copy of the GMRES-coarse param `p` whose LU is the oracle's coarsest solve on p's own coarsest operator and Jacobi vector
    (widened to complex128: a ComplexF32 hierarchy's coarsest solve runs in double)."""
    q = copy.copy(p)
    q.LU = OracleCoarseGmres(p.As[-1], p.LU)
    q.device = None
    return q


# ---- operators ----------------------------------------------------------------------------------------------------------------------
def awkward(n, seed):
    """The construction of _awkward_operator in tests/test_complex_kcycle_gpu.py: complex square CSR with empty rows, rows spanning the
    kernel's 1024-entry chunks and one row longer than a chunk (row 2000: 3000 entries)."""
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


def s100():
    """100 rows in ONE row block."""
    A = (sp.random(100, 100, density=.03, random_state=5) + 1j * sp.random(100, 100, density=.03, random_state=6)).tocsr()
    A.sort_indices()
    return A


def dominant(A, f):
    """A with its diagonal replaced by (f * sum_j |a_ij| + 1)(1 + 0.3i), the sum over every entry of A's row (an old diagonal included)."""
    A = sp.csr_matrix(A, dtype=np.complex128)
    rowsum = np.asarray(abs(A).sum(axis=1)).ravel()
    off = (A - sp.diags(A.diagonal())).tocsr()
    off.eliminate_zeros()
    B = (off + sp.diags((f * rowsum + 1.0) * (1.0 + 0.3j))).tocsr()
    B.sort_indices()
    return B


#            name: (operator, the oracle's steps, whether it breaks)
_SOLVE_OPS = {"awkward5000_f0.3": (lambda: dominant(awkward(5000, 3), 0.3), 10, False),
              "awkward5000_f1.5": (lambda: dominant(awkward(5000, 3), 1.5), 5, True),
              "S100_f1.5": (lambda: dominant(s100(), 1.5), 4, True)}
SOLVE_CASES = tuple(_SOLVE_OPS)
_solve_cache = {}


def solve_case(name):
    """(A_c, d = 0.8 / diag, b = complex_rhs(n, 31), the oracle's coarsest solve with ONE logged call, its x): shared, never modified."""
    if name not in _solve_cache:
        A = _SOLVE_OPS[name][0]()
        d = 0.8 / A.diagonal()
        b = complex_rhs(A.shape[0], 31)
        orc = OracleCoarseGmres(A, d)
        x = orc.solve(b)
        _solve_cache[name] = (A, d, b, orc, x)
    return _solve_cache[name]


def solve_expected(name):
    return _SOLVE_OPS[name][1:]


def manual_param(mg, Ac, seed=7):
    """A two-level complex param (in the manner of _manual_param, tests/test_complex_kcycle_gpu.py) whose COARSEST operator is Ac, with
    the GMRES coarsest solve: LU = 0.8 / diag(Ac).  Only the coarsest solve is run on it: the fine level is a stub of 67 rows (scipy's
    sp.random draws from all n * nc positions, seconds for a fine level above a 5000-row coarsest one)."""
    nc = Ac.shape[0]
    n = 67
    rng = np.random.default_rng(seed)
    A = (sp.identity(n) * (4.0 + 1j) + 0.1 * sp.random(n, n, density=4.0 / n, random_state=seed + 2)).tocsr().astype(np.complex128)
    A.sort_indices()
    P = sp.random(n, nc, density=4.0 / nc, random_state=seed, format="csr")
    R = sp.random(nc, n, density=6.0 / n, random_state=seed + 1, format="csr")
    P.sort_indices()
    R.sort_indices()
    p = mg.getMGparam(np.complex128, np.int64, 2, 8, 4, 1e-10, "Jac", 0.8, 1, 1, "V", "GMRES")
    p.As, p.Ps, p.Rs = [A, Ac], [P], [R]
    p.relaxPrecs = [0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))]
    p.LU = np.ascontiguousarray(0.8 / Ac.diagonal(), dtype=np.complex128)
    p.nrhs = 1
    return p


# ---- hierarchies --------------------------------------------------------------------------------------------------------------------
#         name: (levels, k h, relaxType, cycleType, pre, post)
HIERARCHIES = {"2lev": (2, 0.5, "Jac", "V", 2, 1), "3lev": (3, 0.5, "Jac", "V", 2, 1), "4lev": (4, 0.25, "Jac", "V", 2, 1),
               "3levK": (3, 0.5, "Jac-GMRES", "K", 2, 1)}


def hierarchy(mg, name, coarse="GMRES", maxIter=8, single=False, damping=0.5, relax=None):
    """helmholtz(mg, [16, 16, 16], k h, damping), relaxParam 0.8, set up; a fresh param on every call."""
    levels, kh, rel, cyc, pre, post = HIERARCHIES[name]
    A, mesh = helmholtz(mg, [16, 16, 16], kh, damping)
    kw = {"singlePrecision": True} if single else {}
    p = mg.getMGparam(np.complex128, np.int64, levels, 8, maxIter, 1e-10, relax or rel, 0.8, pre, post, cyc, coarse, 0.5, 0.0, **kw)
    mg.MGsetup(A, mesh, p)
    return p


def cycle_rhs(p):
    return complex_rhs(p.As[0].shape[0], 9)
