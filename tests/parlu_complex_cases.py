"""Shared inputs of the ComplexF64 factor-applier tests (mg_lu_*_CFP64; test infrastructure): the systems, the reference's
compiled applyLUsolve_CFP64_INT64 for blocks of right-hand sides and both solve directions, and its stored outputs
(tests/golden/reference_binaries/parlu_complex_outputs.npz, written by make_parlu_complex_outputs.py beside it)."""
import ctypes as C
import os

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from complex_cases import lu_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "parLU.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_binaries", "parlu_complex_outputs.npz")
PERMC = "MMD_AT_PLUS_A"
NRHS = (1, 5, 6)


def complex_block(n, nrhs, seed):
    """Seeded complex right-hand sides: a vector for nrhs == 1, else n x nrhs column-major (as Julia holds them)."""
    rng = np.random.default_rng(seed)
    if nrhs == 1:
        return rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return np.asfortranarray(rng.standard_normal((n, nrhs)) + 1j * rng.standard_normal((n, nrhs)))


def shifted_laplacian(mg, seed=0):
    """testParallelJuliaSolver.jl:13-21,73: G'*m*G + (1+1im)*I on 20 x 23 cells, seeded."""
    rng = np.random.default_rng(seed)
    Mr = mg.getRegularMesh([0.0, 1.0, 0.0, 1.0], [20, 23])
    G = mg.getNodalGradientMatrix(Mr)
    m = sp.diags(np.exp(rng.standard_normal(G.shape[0])))
    Ar = (G.T @ m @ G).tocsc()
    return (Ar.astype(np.complex128) + (1.0 + 1.0j) * sp.identity(Ar.shape[1])).tocsc()


def _stored_matrix(name):
    """A matrix stored beside the reference's outputs (csc arrays in parlu_complex_outputs.npz): the fixture does not depend
    on how a scipy version draws sp.random."""
    z = np.load(GOLDEN)
    shape = tuple(int(v) for v in z[name + "_shape"])
    return sp.csc_matrix((z[name + "_data"], z[name + "_indices"], z[name + "_indptr"]), shape=shape)


def nonsymmetric50():
    """testParallelJuliaSolver.jl:101-104: a REAL unsymmetric matrix sprandn(n, n, 5/n) + 10*I, n = 50 (stored; drawn by
    make_parlu_complex_outputs.py)."""
    return _stored_matrix("nonsym50_A")


def helmholtz_unsymmetric():
    """A 2-D Helmholtz-like operator on the nodes of 20 x 23 cells with an unsymmetric complex perturbation (the kind
    complex_cases.lu_pin_system builds; stored, drawn by make_parlu_complex_outputs.py): A, A^T and A^H all differ."""
    return _stored_matrix("helmholtz_unsym_A")


def ref_lu_solve_complex_block(lu, B, doTranspose=0, so_path=REF_SO):
    """The reference's applyLUsolve_CFP64_INT64 (parLU.cpp:69-72) on a complex splu in parLU's layout, one factorisation,
    nrhs right-hand sides; doTranspose = 1 is applyLUsolveTrans (parLU.cpp:193-260).  B is copied: the reference uses it
    as work space."""
    lib = C.CDLL(so_path)
    f = lib.applyLUsolve_CFP64_INT64
    i64p, f64p = C.POINTER(C.c_longlong), C.POINTER(C.c_double)
    f.restype = None
    f.argtypes = [i64p, f64p, i64p, i64p, f64p, i64p, i64p, i64p, i64p, i64p, f64p, f64p,
                  C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong]
    F = lu_layout(lu)
    n = lu.shape[0]
    B = np.asfortranarray(B, dtype=np.complex128)
    nrhs = 1 if B.ndim == 1 else B.shape[1]
    nn = np.full(nrhs + 1, n, dtype=np.int64)          # (parLU.cpp:143-145 indexes n by the right-hand side)
    nnz = np.full(nrhs + 1, F["nnz"], dtype=np.int64)
    X = np.zeros_like(B, order="F")
    Bw = B.copy(order="F")
    P = lambda a: a.ctypes.data_as(i64p)
    D = lambda a: a.ctypes.data_as(f64p)
    f(P(F["Lp"]), D(F["Lv"]), P(F["Lc"]), P(F["Up"]), D(F["Uv"]), P(F["Uc"]), P(F["p"]), P(F["q"]), P(nn), P(nnz), D(X), D(Bw),
      1, nrhs, 1, 1, int(doTranspose))
    return X


def pinned_cases():
    """(name, A as complex csc, B, doTranspose) of every stored output: the real unsymmetric matrix of the reference's
    adjoint sequence and the complex unsymmetric operator, plain and adjoint, one and several right-hand sides."""
    cases = []
    A50 = nonsymmetric50().astype(np.complex128).tocsc()
    Ah = helmholtz_unsymmetric()
    for nrhs in (1, 5):
        for t in (0, 1):
            cases.append((f"nonsym50_nrhs{nrhs}_t{t}", A50, complex_block(50, nrhs, 30 + nrhs), t))
    for nrhs in NRHS:
        for t in (0, 1):
            cases.append((f"helmholtz_unsym_nrhs{nrhs}_t{t}", Ah, complex_block(Ah.shape[0], nrhs, 11 + nrhs), t))
    return cases


def reference_solution(name, lu, B, doTranspose):
    """The reference binary's solution where it was built, else its stored output."""
    if os.path.exists(REF_SO):
        return ref_lu_solve_complex_block(lu, B, doTranspose)
    return np.load(GOLDEN)[name]


def factor(A):
    return spla.splu(sp.csc_matrix(A), permc_spec=PERMC)
