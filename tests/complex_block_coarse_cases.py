"""TEST INFRASTRUCTURE ONLY.  The GMRES coarsest solve of a complex hierarchy given a BLOCK of right-hand sides (MGcycle.jl:165-167:
``blockFGMRES(Afun, b, 10, tol = 0.01, maxIter = 1, M = d.*, X = 0)``) as the oracles see it, and the cases its tests share.  Imports
no device code of the package.

``OracleBlockCoarseGmres`` is an object with ``.solve(B)``: ``complex_block_fgmres_oracle.blockFGMRES(A_c., B, 10, 0.01, 1, M = d.*)``;
it logs (flag, steps, resvec) of every call.  A vector goes through as a block of one column.

The WHOLE-BLOCK cycle: with this coarsest solve the columns of a block are coupled (one Krylov space, one stopping test for all of
them), so ``complex_block_oracle.block_cycle``, which runs column by column, is NOT the oracle here.  ``block_cycle`` below is
``complex_oracle.recursiveCycle`` itself on 2-D arrays - relaxPrecs as columns so that ``d * r`` broadcasts over the block, the level
memory n x k, ``norm(x) > 0`` the Frobenius norm of the block - calling that coarsest solve.
tests/test_complex_block_coarse_gmres_host.py shows that the two differ by far more than the tolerance.

``clearance(log)`` is complex_coarse_cases.clearance: every comparison with the device first asserts ON THE ORACLE'S LOG ALONE that
no logged estimate lies within a factor MIN_CLEARANCE = 1.5 of 0.01.  If that fails the input is wrong: change the input, never the
factor."""
from __future__ import annotations

import copy

import numpy as np
import scipy.sparse as sp

import complex_block_fgmres_oracle as bf
import complex_block_oracle as cb
import complex_coarse_cases as cc
import complex_oracle as corc
from complex_cases import helmholtz

CB_STEPS, CB_TOL = 10, 0.01
MIN_CLEARANCE = cc.MIN_CLEARANCE
clearance = cc.clearance


class OracleBlockCoarseGmres:
    def __init__(self, Ac, d):
        self.A = sp.csr_matrix(Ac, dtype=np.complex128)
        self.d = np.asarray(d, dtype=np.complex128).reshape(-1, 1)
        self.log = []
        self.afun = lambda V: self.A @ V            # (a test may wrap it: the noise run)

    def solve(self, B):
        B = np.asarray(B, dtype=np.complex128)
        B2 = B.reshape(-1, 1) if B.ndim == 1 else B
        X, flag, steps, resvec = bf.blockFGMRES(lambda V: self.afun(V), B2, CB_STEPS, CB_TOL, 1, lambda V: self.d * V)
        self.log.append((flag, steps, np.array(resvec)))
        return X.reshape(B.shape)


# ---- the solve alone ----------------------------------------------------------------------------------------------------------------
#   (operator of complex_coarse_cases._SOLVE_OPS, k): (the oracle's steps, its flag).  awkward5000: 5000 rows, no multiple of 256, with
#   empty rows and one row of 3000 entries that feeds every partial; S100: one row block.  k = 3 and 5 are no powers of two.
#   (S100_f1.5 at k = 16 has clearance 1.06: not used.)
SOLVE_RUNS = {}
for _k in (2, 3, 5, 8, 16):
    SOLVE_RUNS[("awkward5000_f0.3", _k)] = (10, -1)
    SOLVE_RUNS[("awkward5000_f1.5", _k)] = (5, 0)
for _k in (2, 3, 5, 8):
    SOLVE_RUNS[("S100_f1.5", _k)] = (4, 0)
ZERO_COLUMN = ("S100_f1.5", 3)      # the block of this run with its middle column zeroed: 4 steps, flag 0, an exactly zero X column
_solve_cache = {}


def solve_rhs(name, k, zero_column=False):
    n = cc.solve_case(name)[0].shape[0]
    B = np.array(cb.block_rhs(n, k))
    if zero_column:
        B[:, k // 2] = 0
    return np.asfortranarray(B)


def solve_case(name, k, zero_column=False):
    """(A_c, d = 0.8 / diag, B, the oracle with ONE logged call, its X): shared, never modified."""
    key = (name, k, zero_column)
    if key not in _solve_cache:
        A, d = cc.solve_case(name)[:2]
        B = solve_rhs(name, k, zero_column)
        orc = OracleBlockCoarseGmres(A, d)
        X = orc.solve(B)
        _solve_cache[key] = (A, d, B, orc, X)
    return _solve_cache[key]


# ---- the whole-block cycle --------------------------------------------------------------------------------------------------------------
class _BlockMem:
    """complex_oracle._Mem for blocks of k columns."""

    def __init__(self, param, k, dtype=np.complex128):
        self.r = [np.zeros((A.shape[0], k), dtype=dtype) for A in param.As]
        self.x = [np.zeros((A.shape[0], k), dtype=dtype) for A in param.As]
        self.b = [np.zeros((A.shape[0], k), dtype=dtype) for A in param.As]
        self.b[-1] = self.r[-1]


def oracle_param(p):
    """A copy of the GMRES-coarse param `p` for the whole-block cycle: LU is the block oracle's coarsest solve on p's own coarsest operator
    and Jacobi vector (complex128: a ComplexF32 hierarchy's coarsest solve runs in double), relaxPrecs are n x 1 columns."""
    q = copy.copy(p)
    q.LU = OracleBlockCoarseGmres(p.As[-1], p.LU)
    q.relaxPrecs = [np.asarray(d).reshape(-1, 1) for d in p.relaxPrecs]
    q.device = None
    return q


def block_cycle(q, B, X):
    """One cycle of the whole block on an oracle_param; returns the new X (a fresh array; B and X are not modified)."""
    B = np.array(B, dtype=np.complex128)
    return np.array(corc.recursiveCycle(q, B, np.array(X, dtype=np.complex128), 1, _BlockMem(q, B.shape[1])))


def block_cycle_single(q, B):
    """The mixed closure of a ComplexF32 hierarchy on the whole block (SolveFuncs.jl:52-58): bl .= B; z .= 0; one cycle of
    tests/complex_single_oracle.py on complex64 blocks (the coarsest solve in double); z widened."""
    import complex_single_oracle as cs
    bl = np.asarray(B, dtype=np.complex128).astype(np.complex64)
    z = np.zeros(bl.shape, dtype=np.complex64)
    return np.array(cs.recursiveCycle(q, bl, z, 1, _BlockMem(q, bl.shape[1], np.complex64))).astype(np.complex128)


def block_solveMG(q, B, X):
    """SolveFuncs.jl:3-39 on the whole block (Frobenius norms); returns (X, iterations, resvec)."""
    A = q.As[0]
    X = np.array(X, dtype=np.complex128)
    res0 = np.linalg.norm(B) if np.linalg.norm(X) == 0 else np.linalg.norm(B - A @ X)
    resvec, it = [res0], 0
    for _ in range(q.maxOuterIter):
        X = block_cycle(q, B, X)
        it += 1
        resvec.append(np.linalg.norm(B - A @ X))
        if resvec[-1] / res0 < q.relativeTol:
            break
    return X, it, np.array(resvec)


# ---- hierarchies: helmholtz of complex_cases, getMGparam(..., "Jac", 0.8, 2, 1, ct, "GMRES", 0.5, 0.0) ----------------------------------
#   name: (grid, levels, k h, damping, cycle).  Clearances over 3 cycles measured on the CPU: 16^3 2 levels (729 coarsest rows) k = 2: 5.2,
#   k = 4: 4.0; 16^3 3 levels damping 0.2 (125 rows) V k = 2: 8.7, k = 4: 3.4, W k = 2: 8.5, k = 4: 2.1; 24^3 3 levels (343 rows) >= 6.7.
#   (The hierarchies of complex_coarse_cases.HIERARCHIES with damping 0.5 on 3 and 4 levels keep only 1.0 - 1.3 with blocks: not used.)
HIERARCHIES = {"16_2lev": ([16] * 3, 2, 0.5, 0.5, "V"), "16_3levV": ([16] * 3, 3, 0.5, 0.2, "V"), "16_3levW": ([16] * 3, 3, 0.5, 0.2, "W"),
               "24_3levV": ([24] * 3, 3, 0.25, 0.2, "V"), "24_3levW": ([24] * 3, 3, 0.25, 0.2, "W")}


def hierarchy(mg, name, maxIter=8, single=False, opt_in=True, damping=None, tol=1e-10):
    """A fresh param, set up; opt_in: blockCoarseGMRES=True."""
    grid, levels, kh, damp, ct = HIERARCHIES[name]
    A, mesh = helmholtz(mg, grid, kh, damp if damping is None else damping)
    kw = {}
    if single:
        kw["singlePrecision"] = True
    if opt_in:
        kw["blockCoarseGMRES"] = True
    p = mg.getMGparam(np.complex128, np.int64, levels, 8, maxIter, tol, "Jac", 0.8, 2, 1, ct, "GMRES", 0.5, 0.0, **kw)
    mg.MGsetup(A, mesh, p)
    return p


def cycle_rhs(p, k):
    return cb.block_rhs(p.As[0].shape[0], k)
