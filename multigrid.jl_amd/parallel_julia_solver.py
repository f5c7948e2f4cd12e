"""Host mirror of src/ParallelJuliaSolver/parallelJuliaSolver.jl: "the host factors, the device applies".

The reference factors with UMFPACK in Julia (``setupLUFactor``, parallelJuliaSolver.jl:113-148) and applies the
triangular factors with its own native code (back end 3: ``applyLUsolve_FP64_INT64``, deps/src/parLU.cpp:52-63,
120-260; one OpenMP task per right-hand side).  Here the factorisation comes from SuperLU (scipy; no UMFPACK in this
image) in the same layout - L and U in CSR, 1-based Int64, L's diagonal last and U's diagonal first, A[p,q] = L*U -
and ``mg_lu_*`` applies them on the GPU, including the solve with the transposed matrix (``doTranspose``).
VAL = ComplexF64 (``applyLUsolve_CFP64_INT64``, the complex Helmholtz systems the module was written for) goes through
``mg_lu_*_CFP64``; there ``doTranspose`` solves with the ADJOINT, x[p] = L^H \\ (U^H \\ b[q]) - Julia's ``A'``.
Single factors - the forms a Helmholtz inversion builds, because the factors are what fills memory - are opt-in:
``getParallelJuliaSolver(VAL, IND, ..., singleFactors=True)`` accepts (Float32, UInt32), (ComplexF32, UInt32) and
(ComplexF32, Int64), the reference's ``applyLUsolve_FP32_UINT32`` / ``_CFP32_UINT32`` / ``_CFP32_INT64``.  The matrix is
factorised in double, as Julia's ``lu`` does for a single matrix (parallelJuliaSolver.jl:114), L and U are converted to VAL
and p, q to IND (l.137-145), and ``mg_lu_*_FP32`` / ``_CFP32`` apply them: stored in single, every row evaluated in double.
Same names and argument meaning as the reference; ``solveLinearSystem_`` is Julia's ``solveLinearSystem!``.
"""
import ctypes as C
import time
from dataclasses import dataclass, field
from typing import Any, Optional

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from . import device as D


@dataclass
class parallelJuliaSolver:
    """parallelJuliaSolver.jl:48-60.  ``backend`` is kept for signature parity (1 native Julia, 2 CSR Julia, 3 CSR C++):
    every value runs the device applier."""
    VAL: Any = np.float64
    IND: Any = np.int64
    L: Optional[sp.csr_matrix] = None
    U: Optional[sp.csr_matrix] = None
    p: Optional[np.ndarray] = None          # 1-based, A[p, q] = L*U
    q: Optional[np.ndarray] = None
    numCores: int = 1
    backend: int = 1
    doClear: int = 0
    nFac: int = 0
    facTime: float = 0.0
    nSolve: int = 0
    solveTime: float = 0.0
    singleFactors: bool = False             # (not in the reference: the opt-in that admits the single forms)
    _handle: Any = field(default=None, repr=False)

    def close(self):
        if self._handle is not None:
            D.load_library().mg_lu_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# (VAL, IND) of the single forms -> the suffix of their create entry point and of their solve entry points
_SINGLE_FORMS = {(np.dtype(np.float32), np.dtype(np.uint32)): ("FP32_UINT32", "FP32"),
                 (np.dtype(np.complex64), np.dtype(np.uint32)): ("CFP32_UINT32", "CFP32"),
                 (np.dtype(np.complex64), np.dtype(np.int64)): ("CFP32_INT64", "CFP32")}


def getParallelJuliaSolver(VAL=np.float64, IND=np.int64, numCores: int = 1, backend: int = 1, *,
                           singleFactors: bool = False) -> parallelJuliaSolver:
    """parallelJuliaSolver.jl:63-70.  ``singleFactors=True`` admits the reference's three single forms, (Float32, UInt32),
    (ComplexF32, UInt32) and (ComplexF32, Int64); without it they are refused as before.  With the keyword the pair must be one
    the reference has: (Float32, Int64), (ComplexF64, UInt32) and (Float64, UInt32) raise.  Without it nothing changes: a Float64
    solver keeps taking any IND, which it never used (its factors go to the device as Int64)."""
    if singleFactors and (np.dtype(VAL), np.dtype(IND)) in _SINGLE_FORMS:
        return parallelJuliaSolver(VAL=VAL, IND=IND, numCores=numCores, backend=backend, singleFactors=True)
    if np.dtype(VAL) in (np.dtype(np.float32), np.dtype(np.complex64)):
        if singleFactors:
            raise TypeError("single factors come as (Float32, UInt32), (ComplexF32, UInt32) or (ComplexF32, Int64): "
                            "the reference has no (%s, %s) form" % (np.dtype(VAL), np.dtype(IND)))
        raise TypeError("only Float64 and ComplexF64 factors are supported on the device path (single factors: singleFactors=True)")
    if np.dtype(VAL) not in (np.dtype(np.float64), np.dtype(np.complex128)):
        raise TypeError("only Float64 and ComplexF64 factors are supported on the device path")
    if np.dtype(VAL) == np.complex128 and np.dtype(IND) != np.int64:
        raise TypeError("ComplexF64 factors take Int64 indices")
    if np.dtype(VAL) == np.float64 and np.dtype(IND) == np.uint32 and singleFactors:
        raise TypeError("Float64 factors take Int64 indices")
    return parallelJuliaSolver(VAL=VAL, IND=IND, numCores=numCores, backend=backend)


def clear_(param: parallelJuliaSolver):
    """``clear!(param)``: drop the factors and the device handle."""
    param.close()
    param.L = param.U = param.p = param.q = None
    param.doClear = 0
    return param


def _is_complex(param: "parallelJuliaSolver") -> bool:
    return np.dtype(param.VAL).kind == "c"


def _single_form(param: "parallelJuliaSolver"):
    """(create suffix, solve suffix) of a single solver, None for a Float64 / ComplexF64 one."""
    return _SINGLE_FORMS.get((np.dtype(param.VAL), np.dtype(param.IND))) if param.singleFactors else None


def _check_dtype(a, param: "parallelJuliaSolver", name: str) -> None:
    """ComplexF64 solver: complex128 arrays only; Float64 solver: no complex array; a single solver: arrays of its VAL only.
    Nothing is cast between them."""
    dt = np.asarray(a).dtype if not sp.issparse(a) else a.dtype
    if _single_form(param):
        if dt != np.dtype(param.VAL):
            raise TypeError(f"{name} has dtype {dt}, but the solver holds {np.dtype(param.VAL)} factors")
    elif _is_complex(param):
        if dt != np.complex128:
            raise TypeError(f"{name} has dtype {dt}, but the solver holds ComplexF64 factors")
    elif dt.kind == "c":
        raise TypeError(f"{name} has dtype {dt}, but the solver holds Float64 factors")


def _upload_factors(param: "parallelJuliaSolver") -> None:
    """(Re)create the device applier from param.L / U / p / q (the layout of setupLUFactor)."""
    lib = D.load_library()
    L, U = param.L, param.U
    VAL = np.dtype(param.VAL)
    a64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
    Lp, Lc, Lv = a64(L.indptr) + 1, a64(L.indices) + 1, np.ascontiguousarray(L.data, dtype=VAL)
    Up, Uc, Uv = a64(U.indptr) + 1, a64(U.indices) + 1, np.ascontiguousarray(U.data, dtype=VAL)
    param.close()
    h = C.c_void_p()
    form = _single_form(param)
    if form:                                      # column indices and permutations in IND, row pointers Int64 as in every form
        IND = np.dtype(param.IND)
        ind = lambda a: np.ascontiguousarray(a, dtype=IND)
        I = D._u32 if IND == np.uint32 else D._i64
        Lc, Uc, p, q = ind(Lc), ind(Uc), ind(param.p), ind(param.q)
        D._check(lib, getattr(lib, "mg_lu_create_" + form[0])(0, L.shape[0], D._i64(Lp), I(Lc), D._f32(Lv), D._i64(Up), I(Uc), D._f32(Uv),
                                                              I(p), I(q), C.byref(h)), "mg_lu_create_" + form[0])
        param._handle = h
        return
    create, what = ((lib.mg_lu_create_CFP64_INT64, "mg_lu_create_CFP64") if _is_complex(param)
                    else (lib.mg_lu_create_FP64_INT64, "mg_lu_create"))
    D._check(lib, create(0, L.shape[0], D._i64(Lp), D._i64(Lc), D._f64(Lv), D._i64(Up), D._i64(Uc), D._f64(Uv),
                         D._i64(param.p), D._i64(param.q), C.byref(h)), what)
    param._handle = h


def copySolver(param: parallelJuliaSolver) -> parallelJuliaSolver:
    """``copySolver`` (parallelJuliaSolver.jl:257-260): copies of L, U, p, q, the settings, counters reset to zero.  The
    copy gets a device applier of its own (created on its first solve) - a set-up solver stays set up."""
    new = getParallelJuliaSolver(param.VAL, param.IND, numCores=param.numCores, backend=param.backend,
                                 singleFactors=param.singleFactors)
    if param.L is not None:
        new.L, new.U = param.L.copy(), param.U.copy()
        new.p, new.q = param.p.copy(), param.q.copy()
    return new


def setupLUFactor(AI, param: parallelJuliaSolver, upload: bool = True) -> parallelJuliaSolver:
    """Factor and convert to the native applier's layout (parallelJuliaSolver.jl:113-148, convertCSC2MyCSR l.26-31).
    upload = False (not in the reference's signature) leaves the device applier to the first solve: the Schwarz sweep
    packs the factors of all its sub-domains into one handle of its own (domain_decomposition.py)."""
    AI = sp.csc_matrix(AI)
    single = _single_form(param) is not None
    if _is_complex(param):
        AI = AI.astype(np.complex128)             # a real matrix through a complex solver (the reference converts too); a single
                                                  # matrix is factorised in double, as Julia's lu does (parallelJuliaSolver.jl:114)
    elif AI.dtype.kind == "c":
        raise TypeError("a complex matrix needs a ComplexF32 solver" if single else "a complex matrix needs a ComplexF64 solver")
    elif single:
        AI = AI.astype(np.float64)
    lu = spla.splu(AI, permc_spec="MMD_AT_PLUS_A")
    L = sp.csr_matrix(lu.L)
    U = sp.csr_matrix(lu.U)
    L.sort_indices()                              # lower: the diagonal is the last entry of every row
    U.sort_indices()                              # upper: the diagonal is the first
    if single:                                    # L, U converted to VAL, p, q to IND (parallelJuliaSolver.jl:137-145)
        L, U = L.astype(np.dtype(param.VAL)), U.astype(np.dtype(param.VAL))
    IND = np.dtype(param.IND) if single else np.dtype(np.int64)
    param.L, param.U = L, U
    param.p = (np.argsort(lu.perm_r) + 1).astype(IND)
    param.q = (np.argsort(lu.perm_c) + 1).astype(IND)
    if upload:
        _upload_factors(param)
    else:
        param.close()
    return param


def setupSolver(AI, param: parallelJuliaSolver) -> parallelJuliaSolver:
    """jInv.LinearSolvers.setupSolver (parallelJuliaSolver.jl:107-110)."""
    return setupLUFactor(AI, param)


def solve(b: np.ndarray, x: np.ndarray, LU: parallelJuliaSolver, doTranspose: int = 0) -> np.ndarray:
    """x[q] = U \\ (L \\ b[p]), or with doTranspose x[p] = L' \\ (U' \\ b[q]) (parallelJuliaSolver.jl:151-207; ' is the
    adjoint for ComplexF64); x is written in place (column-major, as Julia holds it)."""
    _check_dtype(b, LU, "b")
    _check_dtype(x, LU, "x")
    if LU._handle is None:
        if LU.L is None:
            raise RuntimeError("the factors were not set up")
        _upload_factors(LU)          # a copySolver() copy: factors present, device applier not yet created
    lib = D.load_library()
    VAL = np.dtype(LU.VAL)
    bb = np.asfortranarray(b, dtype=VAL)
    if x.dtype != VAL or (x.ndim == 2 and not x.flags.f_contiguous) or not x.flags.writeable:
        raise ValueError("x must be a writable array of the solver's value type in column-major (Julia) layout")
    if bb.shape != x.shape:
        raise ValueError("b and x differ in shape")
    n = bb.shape[0]
    nrhs = 1 if bb.ndim == 1 else bb.shape[1]
    form = _single_form(LU)
    if form:
        what = "mg_lu_solve_" + form[1]
        D._check(lib, getattr(lib, what)(LU._handle, D._f32(bb), D._f32(x), n, nrhs, int(doTranspose)), what)
    elif _is_complex(LU):
        D._check(lib, lib.mg_lu_solve_CFP64(LU._handle, D._f64(bb), D._f64(x), n, nrhs, int(doTranspose)), "mg_lu_solve_CFP64")
    else:
        D._check(lib, lib.mg_lu_solve_FP64(LU._handle, D._f64(bb), D._f64(x), n, nrhs, int(doTranspose)), "mg_lu_solve")
    return x


def solveLinearSystem_(A, B, X: np.ndarray, param: parallelJuliaSolver, doTranspose: int = 0):
    """``solveLinearSystem!(A,B,X,param,doTranspose)`` (parallelJuliaSolver.jl:86-103): factor on first use, then apply."""
    if param.doClear == 1:
        clear_(param)
    if param.L is None:
        t0 = time.perf_counter()
        setupLUFactor(A, param)
        param.facTime += time.perf_counter() - t0
        param.nFac += 1
    if B is not None and np.size(B) > 0:
        if sp.issparse(B):
            B = np.asfortranarray(B.toarray())
        t0 = time.perf_counter()
        X = solve(B, X, param, doTranspose)
        param.solveTime += time.perf_counter() - t0
        param.nSolve += 1
    return X, param


def solveLinearSystem(A, B, param: parallelJuliaSolver, doTranspose: int = 0):
    """``solveLinearSystem(A,B,param,doTranspose)`` (parallelJuliaSolver.jl:75-83): X is a fresh copy of B's shape."""
    _check_dtype(B, param, "B")
    Bd = np.asfortranarray(B.toarray() if sp.issparse(B) else B, dtype=np.dtype(param.VAL))
    return solveLinearSystem_(A, Bd, Bd.copy(order="F"), param, doTranspose)
