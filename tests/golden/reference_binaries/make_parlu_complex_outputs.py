"""Regenerates parlu_complex_outputs.npz beside this file: what the reference's compiled applyLUsolve_CFP64_INT64
(oracle/_ref/parLU.so, built by oracle/Makefile from the reference tree) returns for the cases of
tests/parlu_complex_cases.py::pinned_cases - plain and adjoint solves, one and several right-hand sides - and the two matrices themselves (drawn here with
sp.random, then read by the tests from the file).  Run from the
repository root after the build:
    python tests/golden/reference_binaries/make_parlu_complex_outputs.py"""
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from parlu_complex_cases import GOLDEN, factor, pinned_cases, ref_lu_solve_complex_block  # noqa: E402

def draw_nonsymmetric50(seed=21):
    """sprandn(n, n, 5/n) + 10*I, n = 50 (testParallelJuliaSolver.jl:101-104), real."""
    n = 50
    rng = np.random.default_rng(seed)
    E = sp.random(n, n, density=5.0 / n, random_state=seed, data_rvs=rng.standard_normal, format="csc")
    return (E + 10.0 * sp.identity(n)).tocsc()


def draw_helmholtz_unsymmetric(cells=(20, 23), seed=3):
    T = [sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(c + 1, c + 1)) for c in cells]
    L2 = sp.kronsum(T[0], T[1]).tocsc()
    N = L2.shape[0]
    E = sp.random(N, N, density=3.0 / N, random_state=seed)
    return (L2 - (0.3 - 0.15j) * sp.identity(N) + 0.05j * E).tocsc()


def store_matrix(out, name, A):
    A = sp.csc_matrix(A)
    A.sort_indices()
    out[name + "_data"], out[name + "_indices"], out[name + "_indptr"] = A.data, A.indices, A.indptr
    out[name + "_shape"] = np.array(A.shape, dtype=np.int64)


if __name__ == "__main__":
    out = {}
    if "--keep-matrices" in sys.argv:                       # re-record the outputs for the matrices already stored
        out = {k: v for k, v in np.load(GOLDEN).items() if "_A_" in k}
    else:
        store_matrix(out, "nonsym50_A", draw_nonsymmetric50())
        store_matrix(out, "helmholtz_unsym_A", draw_helmholtz_unsymmetric())
    np.savez_compressed(GOLDEN, **out)                      # pinned_cases() reads the matrices back from the file
    for name, A, B, t in pinned_cases():
        X = ref_lu_solve_complex_block(factor(A), B, t)
        Aop = A.conj().T if t else A
        print(f"{name}: residual {np.abs(Aop @ X - B).max() / np.abs(B).max():.2e}")
        out[name] = X
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN)
