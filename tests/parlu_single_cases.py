"""Shared inputs and comparands of the single-precision factor-applier tests (mg_lu_*_FP32 / _CFP32; test infrastructure;
used by tests/test_parlu_single_host.py, tests/test_parlu_single.py and the generator of
tests/golden/reference_binaries/parlu_single_outputs.npz).

The systems are the stored matrices of the ComplexF64 applier's tests (parlu_complex_cases).  A case's factors come from
scipy's splu in double and are rounded to single, as parallelJuliaSolver.jl:137-145 converts them.  Three evaluations of the
same rounded factors on the same rounded right-hand sides are compared:
  E          the substitution in double (scipy.sparse.linalg.spsolve_triangular on the factors widened back);
  reference  the reference's compiled applyLUsolve_FP32_UINT32 / _CFP32_UINT32 / _CFP32_INT64 (oracle/_ref/parLU.so where it
             is built, its stored outputs otherwise) - single arithmetic, each row summed in stored order;
  device     mg_lu_solve_FP32 / _CFP32.
err(X) = max|X - E| / max|E|.  The device and the reference differ in the order of their sums only, so the yardstick is
err(device) <= 3 * err(reference) (YARDSTICK), with err(reference) <= 1e-5 (REF_ERR_MAX) guarding the fixture."""
import ctypes as C
import os

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from complex_cases import lu_layout
from parlu_complex_cases import NRHS, REF_SO, ROOT, complex_block, factor, helmholtz_unsymmetric

GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_binaries", "parlu_single_outputs.npz")
YARDSTICK = 3.0
REF_ERR_MAX = 1e-5
# form -> (VAL, IND, value-type code of mg_lu_form)
FORMS = {"CFP32_INT64": (np.complex64, np.int64, 3), "CFP32_UINT32": (np.complex64, np.uint32, 3),
         "FP32_UINT32": (np.float32, np.uint32, 2)}
SOLVE = {"CFP32_INT64": "CFP32", "CFP32_UINT32": "CFP32", "FP32_UINT32": "FP32"}


def system(form):
    """The stored 504-row Helmholtz-like operator; its real part (same pattern) for the Float32 form."""
    A = helmholtz_unsymmetric()
    if FORMS[form][0] is np.float32:
        A = sp.csc_matrix((np.ascontiguousarray(A.data.real), A.indices, A.indptr), shape=A.shape)
    return A


def single_block(form, n, nrhs, seed):
    """Seeded right-hand sides in the form's value type: a vector for nrhs == 1, else n x nrhs column-major."""
    B = complex_block(n, nrhs, seed)
    VAL = FORMS[form][0]
    return np.asfortranarray(B.real if VAL is np.float32 else B, dtype=VAL)


def single_layout(lu, form):
    """lu_layout with the values rounded to the form's VAL and the column indices and permutations in its IND (row pointers
    stay Int64, as in every form of the reference)."""
    VAL, IND, _ = FORMS[form]
    F = lu_layout(lu)
    real = VAL is np.float32
    v = lambda a: np.ascontiguousarray(a.real if real else a, dtype=VAL)
    i = lambda a: np.ascontiguousarray(a, dtype=IND)
    return dict(Lp=F["Lp"], Lc=i(F["Lc"]), Lv=v(F["Lv"]), Up=F["Up"], Uc=i(F["Uc"]), Uv=v(F["Uv"]), p=i(F["p"]), q=i(F["q"]),
                nnz=F["nnz"])


def double_substitution(F, B, doTranspose=0):
    """E: x[q] = U \\ (L \\ b[p]), or with doTranspose x[p] = L^H \\ (U^H \\ b[q]), in double on the single factors and the
    single right-hand sides widened back."""
    wide = np.complex128 if F["Lv"].dtype.kind == "c" else np.float64
    n = F["p"].size
    csr = lambda p, c, v: sp.csr_matrix((v.astype(wide), c.astype(np.int64) - 1, p - 1), shape=(n, n))
    L, U = csr(F["Lp"], F["Lc"], F["Lv"]), csr(F["Up"], F["Uc"], F["Uv"])
    p, q = F["p"].astype(np.int64) - 1, F["q"].astype(np.int64) - 1
    Bw = np.asarray(B, dtype=wide)
    X = np.zeros(Bw.shape, dtype=wide, order="F")
    if not doTranspose:
        X[q] = spla.spsolve_triangular(U, spla.spsolve_triangular(L, Bw[p], lower=True), lower=False)
    else:
        UH, LH = sp.csr_matrix(U.conj().T), sp.csr_matrix(L.conj().T)
        X[p] = spla.spsolve_triangular(LH, spla.spsolve_triangular(UH, Bw[q], lower=True), lower=False)
    return X


def err(X, E):
    return float(np.abs(np.asarray(X, dtype=E.dtype) - E).max() / np.abs(E).max())


def ref_lu_solve_single(F, B, form, doTranspose=0, so_path=REF_SO):
    """The reference's applyLUsolve_<form> (parLU.cpp:33-46, 85-115) on factors in single_layout; B is copied: the reference
    uses it as work space."""
    VAL, IND, _ = FORMS[form]
    lib = C.CDLL(so_path)
    f = getattr(lib, "applyLUsolve_" + form)
    i64p, fp = C.POINTER(C.c_longlong), C.POINTER(C.c_float)
    ip = i64p if IND is np.int64 else C.POINTER(C.c_uint)
    f.restype = None
    f.argtypes = [i64p, fp, ip, i64p, fp, ip, ip, ip, i64p, i64p, fp, fp,
                  C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong]
    n = F["p"].size
    B = np.asfortranarray(B, dtype=VAL)
    nrhs = 1 if B.ndim == 1 else B.shape[1]
    nn = np.full(nrhs + 1, n, dtype=np.int64)          # (parLU.cpp:143-145 indexes n by the right-hand side)
    nnz = np.full(nrhs + 1, F["nnz"], dtype=np.int64)
    X = np.zeros_like(B, order="F")
    Bw = B.copy(order="F")
    P = lambda a: a.ctypes.data_as(i64p)
    I = lambda a: a.ctypes.data_as(ip)
    V = lambda a: a.ctypes.data_as(fp)
    f(P(F["Lp"]), V(F["Lv"]), I(F["Lc"]), P(F["Up"]), V(F["Uv"]), I(F["Uc"]), I(F["p"]), I(F["q"]), P(nn), P(nnz), V(X), V(Bw),
      1, nrhs, 1, 1, int(doTranspose))
    return X


_cases = {}


def case(form, nrhs, t):
    """(name, F, B, E) of one yardstick case on the stored Helmholtz-like operator; computed once and shared - nothing in it
    may be modified."""
    k = (form, nrhs, t)
    if k not in _cases:
        A = system(form)
        F = single_layout(factor(A), form)
        B = single_block(form, A.shape[0], nrhs, 11 + nrhs)
        _cases[k] = (f"helmholtz_unsym_{form}_nrhs{nrhs}_t{t}", F, B, double_substitution(F, B, t))
    return _cases[k]


def pinned_cases():
    return [(form, nrhs, t) for form in FORMS for nrhs in NRHS for t in (0, 1)]


def reference_solution(form, nrhs, t):
    """The reference binary's solution where it was built, else its stored output."""
    name, F, B, _ = case(form, nrhs, t)
    if os.path.exists(REF_SO):
        return ref_lu_solve_single(F, B, form, t)
    return np.load(GOLDEN)[name]


def create_args(mg, F, form):
    """The argument tuple of mg_lu_create_<form> behind the device id and n."""
    D = mg.device
    I = D._i64 if FORMS[form][1] is np.int64 else D._u32
    return (D._i64(F["Lp"]), I(F["Lc"]), D._f32(F["Lv"]), D._i64(F["Up"]), I(F["Uc"]), D._f32(F["Uv"]), I(F["p"]), I(F["q"]))


def lu_form(mg, handle, t=0):
    info = np.zeros(7, dtype=np.int64)
    assert mg.device.load_library().mg_lu_form(handle, t, mg.device._i64(info)) == 0
    return dict(kind=int(info[0]), multi=int(info[1]), tail=int(info[2]), launchedL=int(info[3]), launchedU=int(info[4]),
                levelsL=int(info[5]), levelsU=int(info[6]))
