"""TEST INFRASTRUCTURE ONLY.  The shared inputs of tests/test_complex_adjoint_host.py and tests/test_complex_adjoint_gpu.py: the base
operator - helmholtz(cells, k h = 0.5, damping 0.5) plus the one-sided super-diagonal perturbation of tests/test_transpose_device.py,
times 1 + 0.3i: complex, non-symmetric and non-Hermitian -, its three-level hierarchies, and the comparisons of CSR operators."""
import numpy as np
import scipy.sparse as sp

import complex_coarse_cases as cc
from complex_cases import helmholtz


def base_operator(mg, cells=(16, 12, 10)):
    A, mesh = helmholtz(mg, list(cells), 0.5, 0.5)
    n = A.shape[0]
    N = sp.diags([np.linspace(0.05, 0.3, n - 1)], [1], format="csr") * abs(A[0, 0]) * 0.2
    A = ((A + N) * (1.0 + 0.3j)).tocsr()
    A.sort_indices()
    assert abs(A - A.T).max() > 0 and abs(A - A.conj().T).max() > 0
    return A, mesh


def base_param(mg, relax="SPAI", coarse="NoMUMPS", single=False, maxIter=8, tol=1e-10, cells=(16, 12, 10)):
    A, mesh = base_operator(mg, cells)
    kw = {"singlePrecision": True} if single else {}
    p = mg.getMGparam(np.complex128, np.int64, 3, 8, maxIter, tol, relax, 0.8, 2, 1, "V", coarse, 0.5, 0.0, **kw)
    mg.MGsetup(A, mesh, p)
    return p, A, mesh


def adjoint_sorted(M):
    T = M.conj().T.tocsr()
    T.sort_indices()
    return T


def same_csr(M, T):
    return (M.shape == T.shape and M.dtype == T.dtype and np.array_equal(M.indptr, T.indptr) and np.array_equal(M.indices, T.indices)
            and np.array_equal(M.data, T.data))


def oracle_param(p):
    """What tests/complex_oracle.py cycles on: p itself, or for the GMRES coarsest solve a copy whose LU is the oracle's solve."""
    return cc.oracle_param(p) if p.coarseSolveType == "GMRES" else p
