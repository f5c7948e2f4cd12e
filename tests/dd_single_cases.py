"""Shared inputs and comparands of the single-precision Schwarz tests (mg_dd_*_FP32 / _CFP32; test infrastructure; used by
tests/test_dd_single_host.py, tests/test_dd_single_gpu.py and the generator of
tests/golden/reference_binaries/dd_single_outputs.npz).  It reuses dd_cases, complex_cases and parlu_single_cases.

A case is a grid operator, a box decomposition and a seeded right-hand side.  The DATA are rounded once: the operator and b to
single, every sub-domain matrix A[I, I] (of the rounded operator, widened back) factorised by a double splu and the factors
rounded by parlu_single_cases.single_layout - what setupDDSerial keeps for a single DDparam.  Three evaluations of the same
rounded data are compared:
  E          the sweep in double: the residual in double, parlu_single_cases.double_substitution on the widened factors, x in
             double;
  reference  the reference's own arithmetic: the residual formed term by term in VAL in stored order (computeResidualAtIdx,
             DDSerial.jl:4-20), the sub-solve by the reference's compiled applyLUsolve_<form> (ref_lu_solve_single; single
             arithmetic, each row summed in stored order), x[I] += t in single.  Where oracle/_ref/parLU.so is not built, the final
             x of each case is read from the stored file;
  device     solveDDSerial on a single DDparam.
err(X) = max|X - E| / max|E|.  The device and the reference differ in the order and the width of their sums only, so the
yardstick is parlu_single_cases': err(device) <= YARDSTICK * err(reference), after one sweep from zero and again after two
more, with err(reference) <= REF_ERR_MAX guarding the fixture (asserted on every case by tests/test_dd_single_host.py; all
listed cases meet it as they are, none had to be replaced)."""
import os

import numpy as np
import scipy.sparse as sp

import dd_cases
from complex_cases import complex_rhs, helmholtz
from parlu_single_cases import FORMS, REF_ERR_MAX, YARDSTICK, double_substitution, err, ref_lu_solve_single, single_layout  # noqa: F401
from parlu_complex_cases import REF_SO, ROOT, factor

GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_binaries", "dd_single_outputs.npz")

# name -> (operator, cells, boxes, overlap, form, doTranspose).  The shapes are the smallest ones of tests/test_dd_gpu.py.
CASES = {
    "poisson2d_f32": ("poisson", [32, 32], [8, 8], [1, 1], "FP32_UINT32", 0),
    "helmholtz2d_c32_t0": ("helmholtz", [32, 32], [8, 8], [1, 1], "CFP32_INT64", 0),
    "helmholtz2d_c32_t1": ("helmholtz", [32, 32], [8, 8], [1, 1], "CFP32_UINT32", 1),
    "helmholtz3d_c32_t0": ("helmholtz", [16, 16, 8], [4, 4, 2], [1, 1, 1], "CFP32_INT64", 0),
    "helmholtz3d_c32_t1": ("helmholtz", [16, 16, 8], [4, 4, 2], [1, 1, 1], "CFP32_UINT32", 1),
    "poisson3d_f32": ("poisson", [16, 16, 8], [4, 4, 2], [1, 1, 1], "FP32_UINT32", 0),
    "uneven_f32": ("poisson", [34, 30], [4, 4], [1, 1], "FP32_UINT32", 0),
    "dependent_f32": ("poisson", [32, 32], [8, 8], [2, 2], "FP32_UINT32", 0),
    "dependent_c32": ("helmholtz", [32, 32], [8, 8], [2, 2], "CFP32_INT64", 0),
}
SWEEPS = (1, 3)   # the iterates that are compared: after one sweep from zero, and after two more


class Case:
    """The rounded data of one case and its evaluations E and reference, each computed once - nothing in it may be modified."""

    def __init__(self, mg, name):
        op, cells, boxes, overlap, form, t = CASES[name]
        self.name, self.cells, self.boxes, self.overlap, self.form, self.t = name, cells, boxes, overlap, form, t
        self.VAL, self.IND, self.kind = FORMS[form]
        self.wide = np.complex128 if np.dtype(self.VAL).kind == "c" else np.float64
        if op == "poisson":
            A, self.mesh, b = dd_cases.poisson(mg, cells, seed=len(name))
        else:
            A, self.mesh = helmholtz(mg, cells, 0.5, 0.5)
            b = complex_rhs(A.shape[0], seed=len(name))
        self.A = sp.csr_matrix(A).astype(self.VAL)          # the operator the single DDparam is set up on
        self.A.sort_indices()
        self.b = np.ascontiguousarray(b, dtype=self.VAL)
        self.Aw = self.A.astype(self.wide)
        self.lists, self.colors, self.F = [], [], []
        for ii in range(1, int(np.prod(boxes)) + 1):
            loc = mg.cs2loc(ii, boxes)
            I = np.asarray(mg.getNodalIndicesOfCell(boxes, overlap, loc, np.asarray(cells)), dtype=np.int64) - 1
            self.lists.append(I)
            self.colors.append(dd_cases.cell_color(loc))
            self.F.append(single_layout(factor(self.Aw[I][:, I]), form))
        self._E = self._ref = None

    def _members(self):
        for color in range(1, 2 ** len(self.boxes) + 1):
            for I, c, F in zip(self.lists, self.colors, self.F):
                if c == color:
                    yield I, F

    def E(self):
        """{sweeps: x} of the sweep in double on the rounded data."""
        if self._E is None:
            x, bw, out = np.zeros(self.b.size, dtype=self.wide), self.b.astype(self.wide), {}
            for s in range(1, max(SWEEPS) + 1):
                for I, F in self._members():
                    x[I] += double_substitution(F, bw[I] - self.Aw[I] @ x, self.t)
                if s in SWEEPS:
                    out[s] = x.copy()
            self._E = out
        return self._E

    def residual_in_val(self, x, I):
        """computeResidualAtIdx in VAL: r[t] = r[t] - a*x[col], one rounded product and one rounded subtraction per stored
        entry, in stored order (vectorised over the rows, entry position by entry position)."""
        rp, ci, nz = self.A.indptr, self.A.indices, self.A.data
        r = self.b[I].copy()
        start, length = rp[I], rp[I + 1] - rp[I]
        for j in range(int(length.max())):
            rows = np.nonzero(length > j)[0]
            k = start[rows] + j
            r[rows] = r[rows] - nz[k] * x[ci[k]]
        assert r.dtype == self.VAL
        return r

    def reference_sweeps(self):
        """{sweeps: x} by the reference's arithmetic (needs oracle/_ref/parLU.so)."""
        x, out = np.zeros(self.b.size, dtype=self.VAL), {}
        for s in range(1, max(SWEEPS) + 1):
            for I, F in self._members():
                x[I] = x[I] + ref_lu_solve_single(F, self.residual_in_val(x, I), self.form, self.t)
            if s in SWEEPS:
                out[s] = x.copy()
        return out

    def reference(self):
        """The reference's iterates where its binary was built, else its stored ones."""
        if self._ref is None:
            if os.path.exists(REF_SO):
                self._ref = self.reference_sweeps()
            else:
                Z = np.load(GOLDEN)
                self._ref = {s: Z[f"{self.name}_s{s}"] for s in SWEEPS}
        return self._ref

    def dd_param(self, mg):
        """The product's single DDparam on the rounded operator, set up."""
        Ainv = mg.ParallelJuliaSolver.getParallelJuliaSolver(self.VAL, self.IND, singleFactors=True)
        p = mg.getDomainDecompositionParam(self.VAL, np.int64, self.mesh, self.boxes, self.overlap, mg.getNodalIndicesOfCell, Ainv,
                                           singleValues=True)
        return mg.setupDDSerial(self.A, p)


_cases = {}


def case(mg, name):
    if name not in _cases:
        _cases[name] = Case(mg, name)
    return _cases[name]
