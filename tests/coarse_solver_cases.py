"""Shared inputs and comparands of the solver-object coarsest-solve tests (test infrastructure; used by
tests/test_coarse_solver_host.py and tests/test_coarse_solver_gpu.py).

The comparands are the existing restatements - oracle/mg_oracle.py (real) and tests/complex_oracle.py (complex) - given a
shallow copy of the param whose ``LU`` is an adapter with ``.solve(b)``: one sweep of ``dd_cases.Restated`` on the
coarsest matrix from zero (what MGcycle.jl:140-143 does with xc = 0, l.63-64), or scipy's ``splu``."""
import copy

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import dd_cases


class SweepLU:
    """``LU.solve(b)`` = one multiplicative Schwarz sweep from x = 0 with doTranspose = 0 (the restatement of dd_cases)."""

    def __init__(self, mg, param, boxes, overlap):
        self.R = dd_cases.Restated(mg, param.As[-1], np.asarray(param.Meshes[-1].n), boxes, overlap)

    def solve(self, b):
        b = np.asarray(b)
        x = np.zeros(b.size, dtype=np.result_type(self.R.A.dtype, b.dtype))
        return self.R.sweep(b.reshape(-1), x).reshape(b.shape)


class SpluLU:
    """``LU.solve(b)`` = scipy's splu of the coarsest matrix, in its default ordering (not the product's)."""

    def __init__(self, param):
        self.lu = spla.splu(sp.csc_matrix(param.As[-1]))

    def solve(self, b):
        return self.lu.solve(np.asarray(b))


def oracle_param(param, LU):
    """A shallow copy of the param for the restatements: the same hierarchy, ``LU`` replaced by the adapter, no device."""
    q = copy.copy(param)
    q.LU = LU
    q.device = None
    return q


def dd_lu(mg, mesh, boxes, overlap, VAL=np.float64):
    """A DomainDecompositionParam as a caller presets it in ``param.LU``: not set up, parallelJuliaSolver sub-domain solves."""
    Ainv = mg.ParallelJuliaSolver.getParallelJuliaSolver(VAL, np.int64, numCores=2, backend=1)
    return mg.getDomainDecompositionParam(VAL, np.int64, mesh, boxes, overlap, mg.getNodalIndicesOfCell, Ainv)


def pjs_lu(mg, VAL=np.float64):
    return mg.ParallelJuliaSolver.getParallelJuliaSolver(VAL, np.int64, numCores=2, backend=3)


def setup(mg, A, mesh, levels, LU, VAL=np.float64, relax="Jac", omega=0.8, pre=2, post=2, cyc="V", maxIter=12, tol=1e-8):
    """getMGparam + a preset ``LU`` + MGsetup."""
    p = mg.getMGparam(VAL, np.int64, levels, 8, maxIter, tol, relax, omega, pre, post, cyc, "NoMUMPS", 0.5, 0.0)
    p.LU = LU
    mg.MGsetup(A, mesh, p)
    return p


def relmax(x, ref):
    return np.abs(x - ref).max() / np.abs(ref).max()
