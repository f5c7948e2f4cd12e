"""Hybrid Kaczmarz relaxation behind the reference's interface (src/Multigrid/parRelax.jl): ``getHybridKaczmarz``,
``setupHybridKaczmarz``, ``getHybridKaczmarzPrecond``, ``applyHybridKaczmarz``.  The sweeps run on the device
(csrc: hybrid_kaczmarz / hybrid_kaczmarz_c / hybrid_kaczmarz_s <- deps/src/parRelax.h:7-43) through ``mg_kaczmarz_*_FP64``,
for VAL = ComplexF64 ``mg_kaczmarz_*_CFP64`` and, for a param built with ``singleValues=True`` (VAL = Float32 / ComplexF32),
``mg_kaczmarz_*_FP32`` / ``_CFP32``; there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np
import scipy.sparse as sp

from . import device as D
from .dd_indices import getIndicesOfCellsArray, getNodalIndicesOfCell

ArrIdxsType = np.uint32


@dataclass
class hybridKaczmarz:
    """Mirror of ``mutable struct hybridKaczmarz`` (parRelax.jl:8-17)."""
    numDomains: list
    invDiag: Optional[np.ndarray]
    numCores: int
    omega_damp: float
    ArrIdxs: np.ndarray
    precond: Optional[Callable]
    numit: int
    getIndicesOfCell: Callable
    sequential: bool = False            # device schedule: False = one wavefront per sub-domain (the OpenMP analogue)
    _handle: object = field(default=None, repr=False)
    _key: object = field(default=None, repr=False)
    VAL: object = None                  # value type (hybridKaczmarz{VAL}); None: complex128 if invDiag is complex, else float64
    singleValues: bool = False          # opt-in: VAL = float32 / complex64 (VAL = None: complex64 if invDiag is complex, else float32)

    def __post_init__(self):
        cx = self.invDiag is not None and np.iscomplexobj(self.invDiag)
        if self.singleValues:
            if self.VAL is None:
                self.VAL = np.complex64 if cx else np.float32
            if np.dtype(self.VAL) not in (np.dtype(np.float32), np.dtype(np.complex64)):
                raise TypeError(f"hybridKaczmarz: singleValues=True takes VAL = float32 or complex64, not {np.dtype(self.VAL)}")
            self.VAL = np.dtype(self.VAL).type
            return
        if self.VAL is None:
            self.VAL = np.complex128 if cx else np.float64
        if np.dtype(self.VAL).kind == "c" and np.dtype(self.VAL) != np.complex128:
            raise TypeError(f"hybridKaczmarz: VAL = {np.dtype(self.VAL)} is not supported (Float64 or ComplexF64)")

    @property
    def is_complex(self) -> bool:
        return np.dtype(self.VAL).kind == "c"

    @property
    def is_single(self) -> bool:
        return bool(self.singleValues)

    def close(self):
        if self._handle:
            D.load_library().mg_kaczmarz_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def getHybridKaczmarz(VAL, IND, *args, singleValues: bool = False):
    """Both methods of parRelax.jl:24-29 and 39-47: (numDomains, getIndicesOfCell, omega, numCores, numit) leaves the
    setup to ``setupHybridKaczmarz``; (AT, Mesh, numDomains, getIndicesOfCell, omega, numCores, numit) performs it.
    singleValues = True (keyword only, not in the reference's signature) with VAL = np.float32 or np.complex64 builds a
    hybridKaczmarz{Float32} / {ComplexF32} param, served by the reference's FP32 / CFP32 sweeps; any other VAL with it
    raises TypeError.  Without it np.float32 builds a Float64 param and np.complex64 raises TypeError, as they always did."""
    if len(args) == 5:
        numDomains, getIdx, omega, numCores, numit = args
        if singleValues:
            if np.dtype(VAL) not in (np.dtype(np.float32), np.dtype(np.complex64)):
                raise TypeError(f"getHybridKaczmarz: singleValues=True takes VAL = np.float32 or np.complex64, not {np.dtype(VAL)}")
            val = np.dtype(VAL).type
        else:
            val = np.dtype(VAL).type if np.dtype(VAL).kind == "c" else np.float64
        if int(np.prod(numDomains)) < numCores:
            print("*** WARNING: getHybridKaczmarz: numDomains < numCores. ***")
        return hybridKaczmarz(list(numDomains), None, int(numCores), float(omega), np.zeros((1, 1), ArrIdxsType), None,
                              int(numit), getIdx, VAL=val, singleValues=bool(singleValues))
    AT, mesh, numDomains, getIdx, omega, numCores, numit = args
    p = getHybridKaczmarz(VAL, IND, numDomains, getIdx, omega, numCores, numit, singleValues=singleValues)
    return setupHybridKaczmarz(p, AT, mesh)


def _row_sums_in_order(A, vals, dtype=np.float64):
    """sum_k vals_k over each row of the CSR A, added in stored order (one pass per position in the row) in `dtype`."""
    lens = np.diff(A.indptr)
    out = np.zeros(A.shape[0], dtype=dtype)
    for j in range(int(lens.max(initial=0))):
        rows = np.nonzero(lens > j)[0]
        out[rows] += vals[A.indptr[rows] + j]
    return out


def _single_invdiag(A, omega, VAL):
    """invDiag of a Float32 / ComplexF32 param.  Each term conj(a) a is formed in single (complex64: re*re and im*im each
    rounded to float32, then added), a row's terms are added in single in stored order, omega / sum is computed in double
    and rounded to single once."""
    d = A.data
    if np.iscomplexobj(d):
        terms = d.real * d.real + d.imag * d.imag          # float32 arrays: every operation rounded to float32
    else:
        terms = d * d
    assert terms.dtype == np.float32
    s = _row_sums_in_order(A, terms, np.float32)
    return (omega / s.astype(np.float64)).astype(np.float32).astype(VAL)


def setupHybridKaczmarz(param: hybridKaczmarz, AT, mesh):
    """invDiag = convert(Array{VAL,1}, omega ./ sum(conj(AT).*AT, dims=1)) and the index array of the sub-domains
    (parRelax.jl:31-36).  For a complex AT, conj(a) a = re^2 + im^2 exactly, each row's terms are summed in stored order and
    invDiag = omega / sum; a ComplexF64 param stores it as complex128 (zero imaginary part), a Float64 param as float64.
    A single param (singleValues=True) holds AT in its own type (a real AT is cast to it; a complex one on a Float32 param
    raises TypeError): the terms and the row sums are formed in single in stored order, omega / sum in double, rounded to
    single once and stored as float32 / complex64.  That is a reading of parRelax.jl:33 for a single AT (Julia forms
    conj(AT).*AT and its column sums in AT's type and divides the Float64 omega by them); it has not been compared with a
    Julia run."""
    A = sp.csr_matrix(AT)                     # this package holds the CSR of A where Julia holds the CSC of A' (MGdef.jl:75-77)
    if param.is_single:
        if np.iscomplexobj(A.data) and not param.is_complex:
            raise TypeError(f"hybridKaczmarz{{Float32}}: AT is {A.dtype}; build the param with VAL = np.complex64")
        param.invDiag = _single_invdiag(A.astype(param.VAL), param.omega_damp, param.VAL)
    elif np.iscomplexobj(A.data):
        invd = param.omega_damp / _row_sums_in_order(A, A.data.real * A.data.real + A.data.imag * A.data.imag)
        param.invDiag = invd.astype(np.complex128) if param.is_complex else invd
    else:
        invd = param.omega_damp / np.asarray(A.multiply(A).sum(axis=1)).ravel()
        param.invDiag = invd.astype(np.complex128) if param.is_complex else invd
    param.ArrIdxs = getIndicesOfCellsArray(mesh, np.zeros(len(param.numDomains), dtype=np.int64), param.numDomains,
                                           param.getIndicesOfCell)
    param.close()
    return param


def _cheap_key(A):
    """What a call can check for nothing: the object, its buffers and its shape.  A matrix converted on every call (CSC in,
    CSR needed) never matches and pays the full key below - callers that sweep in a loop should hand over a CSR matrix."""
    if not sp.isspmatrix_csr(A):
        return None
    return (id(A), A.data.ctypes.data, A.indices.ctypes.data, A.indptr.ctypes.data, A.nnz, A.shape)


def _matrix_key(A):
    """Identity of the VALUES and of the PATTERN (row pointers included: equal data / indices with other row splits are
    another matrix): the reference passes AT.nzval on every call (parRelax.jl:61-64), so a matrix modified in place, or a
    new one allocated at a recycled id, must not hit the uploaded copy."""
    import zlib
    return (A.nnz, A.shape, zlib.crc32(np.ascontiguousarray(A.data).view(np.uint8)),
            zlib.crc32(np.ascontiguousarray(A.indices).view(np.uint8)), zlib.crc32(np.ascontiguousarray(A.indptr).view(np.uint8)))


def _check_types(param: hybridKaczmarz, **arrays):
    """The reference dispatches applyHybridKaczmarz on hybridKaczmarz{VAL} with AT, r and x of that VAL (parRelax.jl:59-75):
    a Float64 param takes no complex array (its imaginary part would be dropped), a ComplexF64 param only complex128 and a
    single param (Float32 / ComplexF32) only arrays of exactly its type."""
    for name, a in arrays.items():
        dt = np.dtype(a.dtype)
        if param.is_single:
            if dt != np.dtype(param.VAL):
                raise TypeError(f"hybridKaczmarz{{{'ComplexF32' if param.is_complex else 'Float32'}}}: {name} is {dt}, "
                                f"expected {np.dtype(param.VAL)}")
        elif param.is_complex and dt != np.complex128:
            raise TypeError(f"hybridKaczmarz{{ComplexF64}}: {name} is {dt}, expected complex128")
        elif not param.is_complex and dt.kind == "c":
            raise TypeError(f"hybridKaczmarz{{Float64}}: {name} is {dt}; build the param with VAL = np.complex128")


def _device_handle(param: hybridKaczmarz, A, values_changed: bool = True):
    """The uploaded copy of A, re-used while A is the same matrix.  values_changed = False: the caller vouches that a CSR
    matrix with the same buffers as last time still holds the same values (skips the O(nnz) hash of every call).
    A ComplexF64 param uploads conj(A.data), the reference's AT.nzval (AT = A'), and a complex invDiag; a single param
    uploads float32 / complex64 values (conj(A.data) for complex64) and never narrows a double matrix: it refuses it."""
    if param.is_single:
        _check_types(param, AT=A)
    cheap = _cheap_key(A)
    if param._handle is not None and cheap is not None and cheap == getattr(param, "_cheap", None) and not values_changed:
        return param._handle
    Ac = A if sp.isspmatrix_csr(A) else sp.csr_matrix(A)      # converted ONCE: key and upload use the same CSR
    key = _matrix_key(Ac)
    if param._handle is not None and param._key == key:
        param._cheap = cheap
        return param._handle
    param.close()
    lib = D.load_library()
    A = Ac.copy() if not Ac.has_sorted_indices else Ac
    A.sort_indices()
    cp = np.ascontiguousarray(A.indptr, dtype=np.int64) + 1
    rv = np.ascontiguousarray(A.indices, dtype=np.int64) + 1
    arr = np.asfortranarray(param.ArrIdxs, dtype=np.uint32)
    h = C.c_void_p()
    if param.is_single:
        nz = np.ascontiguousarray(np.conj(A.data) if param.is_complex else A.data, dtype=param.VAL)
        invd = np.ascontiguousarray(param.invDiag, dtype=param.VAL)
        sfx = "CFP32" if param.is_complex else "FP32"
        D._check(lib, getattr(lib, f"mg_kaczmarz_create_{sfx}_INT64")(
            0, A.shape[0], D._i64(cp), D._f32(nz), D._i64(rv), arr.shape[1], arr.shape[0],
            arr.ctypes.data_as(C.POINTER(C.c_uint)), D._f32(invd), C.byref(h)), f"mg_kaczmarz_create_{sfx}")
        param._handle, param._key, param._cheap = h, key, cheap
        return h
    if param.is_complex:
        nz = np.ascontiguousarray(np.conj(A.data), dtype=np.complex128)
        invd = np.ascontiguousarray(param.invDiag, dtype=np.complex128)
        create, what = lib.mg_kaczmarz_create_CFP64_INT64, "mg_kaczmarz_create_CFP64"
    else:
        nz = np.ascontiguousarray(A.data, dtype=np.float64)
        invd = np.ascontiguousarray(param.invDiag, dtype=np.float64)
        create, what = lib.mg_kaczmarz_create_FP64_INT64, "mg_kaczmarz_create"
    D._check(lib, create(0, A.shape[0], D._i64(cp), D._f64(nz), D._i64(rv), arr.shape[1], arr.shape[0],
                         arr.ctypes.data_as(C.POINTER(C.c_uint)), D._f64(invd), C.byref(h)), what)
    param._handle, param._key, param._cheap = h, key, cheap
    return h


def applyHybridKaczmarz(param: hybridKaczmarz, AT, r: np.ndarray, x: np.ndarray, numDomains: Optional[int] = None,
                        values_changed: bool = True):
    """``numit`` sweeps of x towards AT' x = r, in place (parRelax.jl:59-65).  values_changed = False (not in the reference's
    signature): the CSR matrix handed over is unchanged since the last call - the uploaded copy is reused without hashing it.
    A ComplexF64 param (parRelax.jl:71-74) takes complex128 AT, r and x, and raises TypeError on any other before the device."""
    _check_types(param, AT=AT, r=np.asarray(r), x=x)
    h = _device_handle(param, AT, values_changed)
    lib = D.load_library()
    if x.ndim == 2 and not x.flags.f_contiguous:
        raise ValueError("x must be column-major (Julia layout)")
    seq = 1 if param.sequential else 0
    if param.is_single:
        rr = np.asfortranarray(r, dtype=param.VAL)
        if x.shape != rr.shape or rr.ndim not in (1, 2) or rr.shape[0] != AT.shape[0] or not (x.flags.f_contiguous and x.flags.writeable):
            raise ValueError(f"x and r must be n or n x nrhs column-major {np.dtype(param.VAL)} arrays of one shape (x writable)")
        nrhs = 1 if rr.ndim == 1 else rr.shape[1]
        sfx = "CFP32" if param.is_complex else "FP32"
        D._check(lib, getattr(lib, f"mg_kaczmarz_apply_{sfx}")(h, D._f32(x), D._f32(rr), nrhs, int(param.numit), seq),
                 f"mg_kaczmarz_apply_{sfx}")
        return x
    if param.is_complex:
        rr = np.asfortranarray(r, dtype=np.complex128)
        if x.shape != rr.shape or rr.shape[0] != AT.shape[0] or not (x.flags.f_contiguous and x.flags.writeable):
            raise ValueError("x and r must be n or n x nrhs column-major complex128 arrays of one shape (x writable)")
        nrhs = 1 if rr.ndim == 1 else rr.shape[1]
        D._check(lib, lib.mg_kaczmarz_apply_CFP64(h, D._f64(x), D._f64(rr), nrhs, int(param.numit), seq), "mg_kaczmarz_apply_CFP64")
        return x
    rr = np.asfortranarray(r, dtype=np.float64)
    nrhs = 1 if rr.ndim == 1 else rr.shape[1]
    D._check(lib, lib.mg_kaczmarz_apply_FP64(h, D._f64(x), D._f64(rr), nrhs, int(param.numit), seq),
             "mg_kaczmarz_apply")
    return x


def getHybridKaczmarzPrecond(param: hybridKaczmarz, AT, nrhs: int):
    """r -> x with x = 0 on entry (parRelax.jl:49-57); the returned closure reuses one buffer, as the reference does."""
    _check_types(param, AT=AT)
    n = AT.shape[1]
    vt = param.VAL if param.is_single else np.complex128 if param.is_complex else np.float64
    x = np.zeros(n, dtype=vt) if nrhs == 1 else np.zeros((n, nrhs), dtype=vt, order="F")

    Ac = AT if sp.isspmatrix_csr(AT) else sp.csr_matrix(AT)   # (converted once for every application of the closure)
    _device_handle(param, Ac, True)

    def precond(r):
        x[...] = 0.0
        # (the reference hands AT.nzval over on every call: values modified in place are honoured unless the caller set
        # param.static_matrix = True, which skips the O(nnz) hash of every application)
        applyHybridKaczmarz(param, Ac, r, x, values_changed=not getattr(param, "static_matrix", False))
        return x

    param.precond = precond
    return precond
