"""Host mirror of src/DomainDecomposition: the overlapping, 2^dim-coloured, multiplicative Schwarz preconditioner whose
sub-domain solves go through ``parallelJuliaSolver`` (DomainDecomposition.jl, DDSerial.jl).  Same names and argument
meaning as the reference: ``cellColor`` (Vanka.jl:105-130), ``DomainDecompositionParam`` /
``getDomainDecompositionParam`` (DomainDecomposition.jl:28-48), ``setupDDSerial`` (DDSerial.jl:81-106),
``solveDDSerial`` (DDSerial.jl:108-139) and ``getDDpreconditioner`` (DomainDecomposition.jl:136-146).

The host factors every sub-domain matrix A[IIp, IIp] (SuperLU in parLU's layout, parallel_julia_solver.setupLUFactor);
the sweeps run on the device through ``mg_dd_*``: the sub-domains of a colour that touch no common entry of x are one
launch, the others run one after another.  There is no CPU fallback.  ``A`` is the applied operator as scipy CSR - what
``param.As[l]`` holds in this package where Julia holds the CSC of A' (MGdef.jl:75-77).

Not mirrored: the operator-constructor / Dirichlet-mass branch (DDSerial.jl:42-61), DDParallel.jl, ``solveGSDDSerial``,
and the reference's ``solveLinearSystem!`` for a ``DomainDecompositionParam`` (it calls an undefined ``Prec`` at this commit,
DomainDecomposition.jl:126-129).  A ``DomainDecompositionParam`` preset as ``param.LU`` of a hierarchy is its coarsest
solve (MGsetup.jl:323-326, MGcycle.jl:140-143): mgsetup.defineCoarsestAinv sets it up, the device hierarchy borrows
its handle.

Single values are opt-in: ``getDomainDecompositionParam(np.float32 | np.complex64, IND, ..., singleValues=True)`` with a
``getParallelJuliaSolver(..., singleFactors=True)`` sub-domain solver of the same VAL.  The reference's param is generic in VAL
(DomainDecomposition.jl:28-48) and its residual and sub-solves run in VAL (DDSerial.jl:4-20, 183-187).  Here the operator, the
factors (factorised in double, then rounded, as setupLUFactor does for single solvers), b, x and the work vectors are STORED in
single - half the HBM of a double sweep - and every residual row and triangular row is EVALUATED in double with one rounding on
the store: a deliberate deviation from the reference, which sums in VAL (the single factor applier's contract).  Nothing is
converted for the caller: A, b and x must be of exactly the param's dtype.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Any, Callable, List, Optional

import numpy as np
import scipy.sparse as sp

from . import device as D
from . import parallel_julia_solver as PJS
from .dd_indices import cs2loc, getNodalIndicesOfCell
from .par_relax import _matrix_key

DDIndType = np.uint32


def cellColor(i) -> int:
    """Colour of the sub-domain with per-dimension (1-based) index i: 1..4 in 2-D, 1..8 in 3-D (Vanka.jl:105-130)."""
    i = [int(k) for k in i]
    if len(i) == 2:
        if i[0] % 2 == 1:
            return 1 if i[1] % 2 == 1 else 2
        return 3 if i[1] % 2 == 1 else 4
    if i[0] % 2 == 1:
        if i[1] % 2 == 1:
            return 1 if i[2] % 2 == 1 else 2
        return 3 if i[2] % 2 == 1 else 4
    if i[1] % 2 == 1:
        return 5 if i[2] % 2 == 1 else 6
    return 7 if i[2] % 2 == 1 else 8


@dataclass
class DomainDecompositionPreconditionerParam:
    """DomainDecomposition.jl:20-26.  With a ``parallelJuliaSolver`` the sub-domain matrix is dropped after the
    factorisation (DDSerial.jl:35-37): ``A_i`` is the empty matrix."""
    sub_problem_param: Any
    i: np.ndarray
    A_i: Any
    DirichletMass: np.ndarray
    Ainv: Any


@dataclass
class DomainDecompositionParam:
    """DomainDecomposition.jl:28-45 (the fields the serial sparse-matrix branch uses)."""
    VAL: Any
    IND: Any
    Mesh: Any
    numDomains: List[int]
    overlap: List[int]
    getIndicesOfCell: Callable = getNodalIndicesOfCell
    Ainv: Any = None
    PrecParams: list = field(default_factory=list)
    GlobalIndices: list = field(default_factory=list)
    doClear: int = 0
    nFac: int = 0
    facTime: float = 0.0
    nSolve: int = 0
    solveTime: float = 0.0
    singleValues: bool = False              # (not in the reference: the opt-in that admits VAL = Float32 / ComplexF32)
    _handle: Any = field(default=None, repr=False)
    _key: Any = field(default=None, repr=False)
    _borrowers: list = field(default_factory=list, repr=False)   # device hierarchies whose coarsest solve is this handle

    @property
    def is_complex(self) -> bool:
        return np.dtype(self.VAL).kind == "c"

    @property
    def is_single(self) -> bool:
        return np.dtype(self.VAL) in _SINGLE_VALS

    def close(self):
        for h in list(self._borrowers):      # an attached handle cannot be destroyed: the hierarchies give it back first
            h._detach_dd()
        if self._handle is not None:
            D.load_library().mg_dd_destroy(self._handle)
            self._handle = None
            self._key = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_SINGLE_VALS = (np.dtype(np.float32), np.dtype(np.complex64))


def getDomainDecompositionParam(VAL, IND, Mesh, numDomains, overlap, getIndicesOfCell=getNodalIndicesOfCell, Ainv=None, *,
                                singleValues: bool = False):
    """DomainDecomposition.jl:46-48.  ``singleValues=True`` (keyword-only, not in the reference's signature) admits VAL = Float32 /
    ComplexF32; without it they are refused as before, and with a double VAL the keyword is refused (as getHybridKaczmarz does)."""
    if singleValues:
        if np.dtype(VAL) not in _SINGLE_VALS:
            raise TypeError("singleValues=True takes VAL = Float32 or ComplexF32, not %s" % np.dtype(VAL))
    elif np.dtype(VAL) not in (np.dtype(np.float64), np.dtype(np.complex128)):
        raise TypeError("only Float64 and ComplexF64 are supported on the device path"
                        + (" (single values: singleValues=True)" if np.dtype(VAL) in _SINGLE_VALS else ""))
    return DomainDecompositionParam(VAL, IND, Mesh, [int(k) for k in numDomains], [int(k) for k in overlap], getIndicesOfCell, Ainv,
                                    singleValues=bool(singleValues))


def copySolver(p: DomainDecompositionParam) -> DomainDecompositionParam:
    """DomainDecomposition.jl:75-78: the settings and a copy of the sub-domain solver, without the setup."""
    Ainv = PJS.copySolver(p.Ainv) if isinstance(p.Ainv, PJS.parallelJuliaSolver) else p.Ainv
    return getDomainDecompositionParam(p.VAL, p.IND, p.Mesh, p.numDomains, p.overlap, p.getIndicesOfCell, Ainv,
                                       singleValues=p.singleValues)


def clear_(p: DomainDecompositionParam) -> DomainDecompositionParam:
    """``clear!(param)`` (DomainDecomposition.jl:59-67 names a field that does not exist; its intent): drop the sub-domain
    factors, the index lists and the device handle; the settings stay."""
    p.close()
    p.PrecParams = []
    p.GlobalIndices = []
    p.doClear = 0
    return p


def isempty(p: DomainDecompositionParam) -> bool:
    """DomainDecomposition.jl:69-72."""
    return len(p.PrecParams) == 0


def setupDDSerial(A, DDparam: DomainDecompositionParam) -> DomainDecompositionParam:
    """DDSerial.jl:81-106, sparse-matrix branch: the index list and the factored matrix A[IIp, IIp] of every sub-domain.
    ``Ainv`` must be a ``parallelJuliaSolver`` of DDparam's VAL (the sub-domain solver the device sweep applies).  A single
    DDparam: ``Ainv`` a ``getParallelJuliaSolver(..., singleFactors=True)`` object of that VAL in one of its three forms, ``A`` a
    scipy matrix of exactly that dtype (TypeError otherwise: the caller converts); every A[IIp, IIp] is factorised in double and the
    factors rounded to VAL (setupLUFactor)."""
    Ainv = DDparam.Ainv
    if not isinstance(Ainv, PJS.parallelJuliaSolver):
        raise NotImplementedError("the device Schwarz sweep applies parallelJuliaSolver factors: Ainv is %s" % type(Ainv).__name__)
    if not sp.issparse(A):
        raise NotImplementedError("the operator-constructor branch (DDSerial.jl:42-61, 97-99) is not mirrored: A must be sparse")
    if np.dtype(Ainv.VAL) != np.dtype(DDparam.VAL):
        raise NotImplementedError("Ainv holds %s factors, DDparam is of %s" % (np.dtype(Ainv.VAL), np.dtype(DDparam.VAL)))
    if DDparam.is_single:
        if PJS._single_form(Ainv) is None:
            raise TypeError("a single DDparam needs a getParallelJuliaSolver(%s, UInt32%s, singleFactors=True) sub-domain solver"
                            % (np.dtype(DDparam.VAL), " or Int64" if DDparam.is_complex else ""))
        if A.dtype != np.dtype(DDparam.VAL):
            raise TypeError("A has dtype %s, but DDparam is of %s: convert it first" % (A.dtype, np.dtype(DDparam.VAL)))
    if A.dtype.kind == "c" and not DDparam.is_complex:
        raise TypeError("a complex operator needs VAL = ComplexF64 (DDparam and its Ainv are Float64)")
    A = sp.csr_matrix(A)
    n = np.asarray(DDparam.Mesh.n, dtype=np.int64)
    numDomains = DDparam.numDomains
    DDparam.close()
    precs, gidx = [], []
    for ii in range(1, int(np.prod(numDomains)) + 1):
        i = cs2loc(ii, numDomains)
        IIp = np.asarray(DDparam.getIndicesOfCell(numDomains, DDparam.overlap, i, n), dtype=np.int64)
        AI = A[IIp - 1][:, IIp - 1]
        sub = PJS.setupLUFactor(AI, PJS.copySolver(Ainv), upload=False)   # (the factors go to the device with the sweep's handle)
        precs.append(DomainDecompositionPreconditionerParam([], i, sp.csc_matrix((0, 0)), np.zeros(0, dtype=DDparam.VAL), sub))
        gidx.append(IIp.astype(DDIndType))
    DDparam.PrecParams = precs
    DDparam.GlobalIndices = gidx
    return DDparam


def coloursIndependent(A, DDparam: DomainDecompositionParam) -> dict:
    """colour -> True where the members of that colour may run as one launch (not in the reference; the host statement of
    the rule ``mg_dd_finalize`` applies): their index sets are pairwise disjoint and no row listed by one member stores a
    column listed by another, so no member reads or writes an entry of x that another member writes."""
    A = sp.csr_matrix(A)
    colours = np.array([cellColor(p.i) for p in DDparam.PrecParams])
    out = {}
    for c in np.unique(colours):
        members = np.nonzero(colours == c)[0]
        rows = np.concatenate([DDparam.GlobalIndices[m].astype(np.int64) - 1 for m in members])
        who = np.concatenate([np.full(len(DDparam.GlobalIndices[m]), k) for k, m in enumerate(members)])
        if len(np.unique(rows)) != len(rows):
            out[int(c)] = False
            continue
        owner = np.full(A.shape[0], -1, dtype=np.int64)
        owner[rows] = who
        listed = A[rows]                                         # the rows the members read, in the order of `who`
        col_owner = owner[listed.indices]
        out[int(c)] = not np.any((col_owner >= 0) & (col_owner != np.repeat(who, np.diff(listed.indptr))))
    return out


def _sfx(DDparam: DomainDecompositionParam) -> str:
    """The suffix of the entry points that serve DDparam's VAL."""
    return {np.dtype(np.float64): "FP64", np.dtype(np.complex128): "CFP64", np.dtype(np.float32): "FP32",
            np.dtype(np.complex64): "CFP32"}[np.dtype(DDparam.VAL)]


def _device_handle(DDparam: DomainDecompositionParam, A):
    """The uploaded sweep (operator, index lists, colours, factors), re-used while A is the same matrix."""
    if isempty(DDparam):
        raise RuntimeError("DDparam is not set up: call setupDDSerial first")
    Ac = A if sp.isspmatrix_csr(A) else sp.csr_matrix(A)
    if Ac.dtype.kind == "c" and not DDparam.is_complex:
        raise TypeError("a complex operator needs VAL = ComplexF64")
    if DDparam.is_single and Ac.dtype != np.dtype(DDparam.VAL):
        raise TypeError("A has dtype %s, but DDparam is of %s: convert it first" % (Ac.dtype, np.dtype(DDparam.VAL)))
    key = _matrix_key(Ac)
    if DDparam._handle is not None and DDparam._key == key:
        return DDparam._handle
    DDparam.close()
    lib = D.load_library()
    VAL = np.dtype(DDparam.VAL)
    cx = DDparam.is_complex
    a64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
    rp, ci, nz = a64(Ac.indptr) + 1, a64(Ac.indices) + 1, np.ascontiguousarray(Ac.data, dtype=VAL)
    idxptr = a64(np.concatenate(([0], np.cumsum([len(g) for g in DDparam.GlobalIndices])))) + 1
    idx = np.ascontiguousarray(np.concatenate(DDparam.GlobalIndices), dtype=DDIndType)
    color = a64([cellColor(p.i) for p in DDparam.PrecParams])
    h = C.c_void_p()
    sfx = _sfx(DDparam)
    val = D._f32 if DDparam.is_single else D._f64
    D._check(lib, getattr(lib, "mg_dd_create_%s_INT64" % sfx)(0, Ac.shape[0], D._i64(rp), D._i64(ci), val(nz), len(color), D._i64(idxptr),
                                                              idx.ctypes.data_as(C.POINTER(C.c_uint)), D._i64(color), C.byref(h)),
             "mg_dd_create_" + sfx)
    try:
        for ic, prec in enumerate(DDparam.PrecParams, start=1):
            s = prec.Ainv
            L, U = s.L, s.U
            # column indices and permutations in the solver's IND for the single forms (parLU has (Float32, UInt32), (ComplexF32, UInt32)
            # and (ComplexF32, Int64)), Int64 for the double ones; row pointers Int64 in every form
            IND = np.dtype(s.IND) if DDparam.is_single else np.dtype(np.int64)
            ind = lambda a: np.ascontiguousarray(a, dtype=IND)
            I = D._u32 if IND == np.uint32 else D._i64
            what = "mg_dd_set_factor_%s_%s" % (sfx, "UINT32" if IND == np.uint32 else "INT64")
            Lp, Lc, Lv = a64(L.indptr) + 1, ind(a64(L.indices) + 1), np.ascontiguousarray(L.data, dtype=VAL)
            Up, Uc, Uv = a64(U.indptr) + 1, ind(a64(U.indices) + 1), np.ascontiguousarray(U.data, dtype=VAL)
            D._check(lib, getattr(lib, what)(h, ic, L.shape[0], D._i64(Lp), I(Lc), val(Lv), D._i64(Up), I(Uc), val(Uv),
                                             I(ind(s.p)), I(ind(s.q))), what)
        D._check(lib, lib.mg_dd_finalize(h), "mg_dd_finalize")
    except Exception:
        lib.mg_dd_destroy(h)
        raise
    DDparam._handle, DDparam._key = h, key
    return h


def ddInfo(DDparam: DomainDecompositionParam, A) -> dict:
    """What ``mg_dd_info`` reports for the sweep on A (not in the reference): how the colours are run."""
    h = _device_handle(DDparam, A)
    lib = D.load_library()
    info = (C.c_longlong * 6)()
    D._check(lib, lib.mg_dd_info(h, info), "mg_dd_info")
    kind = int(info[0])                                          # 0 Float64, 1 ComplexF64, 2 Float32, 3 ComplexF32
    VAL = (np.float64, np.complex128, np.float32, np.complex64)[kind]
    return dict(complex=kind in (1, 3), single=kind in (2, 3), VAL=VAL, numSub=int(info[1]), colours=int(info[2]), batched=int(info[3]), sequential=int(info[4]),
                launches_per_sweep=int(info[5]))


def solveDDSerial(A, b, x, DDparam: DomainDecompositionParam, niter: int = 1, doTranspose: int = 0):
    """``niter`` multiplicative Schwarz sweeps on x, in place (DDSerial.jl:108-139): for every colour, for every
    sub-domain of that colour in linear order, r = (b - A x)[IIp]; t = A_i \\ r; x[IIp] += t.  ``doTranspose`` reaches the
    sub-domain solves only (l.128).  b and x: one right-hand side, numpy vectors of DDparam's VAL - or torch tensors on
    the GPU, swept where they are.  A single DDparam takes b and x of exactly its dtype (numpy float32 / complex64, or
    torch.float32 / torch.complex64 device tensors) and refuses everything else before the device is touched.
    Returns (x, DDparam)."""
    VAL = np.dtype(DDparam.VAL)
    sfx = _sfx(DDparam)
    if DDparam.is_single and not (hasattr(x, "data_ptr") and hasattr(b, "data_ptr")):
        for name, a in (("b", b), ("x", x)):
            if not isinstance(a, np.ndarray) or a.dtype != VAL:
                raise TypeError(f"{name} must be a numpy array (or, with the other vector, a device tensor) of {VAL}: "
                                f"got {getattr(a, 'dtype', type(a).__name__)}")
    if hasattr(x, "data_ptr"):                                   # device-resident vectors
        import torch
        tdt = {"FP64": torch.float64, "CFP64": torch.complex128, "FP32": torch.float32, "CFP32": torch.complex64}[sfx]
        if b.dtype != tdt or x.dtype != tdt:
            raise TypeError("b and x must be %s tensors" % tdt)
        if b.dim() != 1 or x.dim() != 1 or b.numel() != A.shape[0] or x.numel() != A.shape[0]:
            raise ValueError("b and x must be vectors of length %d (one right-hand side)" % A.shape[0])
        h = _device_handle(DDparam, A)
        lib = D.load_library()
        D._sync_torch(b, x)
        D._check(lib, getattr(lib, "mg_dd_apply_dev_" + sfx)(h, D._ptr(b), D._ptr(x), A.shape[0], int(niter), int(doTranspose)),
                 "mg_dd_apply_dev_" + sfx)
        return x, DDparam
    bb = np.asarray(b)
    for name, a in (("b", bb), ("x", x)) if not DDparam.is_single else ():   # (a single param's vectors were checked above)
        if DDparam.is_complex and a.dtype != np.complex128:
            raise TypeError(f"{name} has dtype {a.dtype}, but DDparam is of ComplexF64")
        if not DDparam.is_complex and a.dtype.kind == "c":
            raise TypeError(f"{name} has dtype {a.dtype}, but DDparam is of Float64")
    if bb.ndim != 1 or x.ndim != 1 or bb.shape[0] != A.shape[0] or x.shape != bb.shape:
        raise ValueError("b and x must be vectors of length %d (one right-hand side: the reference indexes b[Idxs])" % A.shape[0])
    if x.dtype != VAL or not (x.flags.c_contiguous and x.flags.writeable):
        raise ValueError("x must be a writable contiguous vector of DDparam's value type")
    bb = np.ascontiguousarray(bb, dtype=VAL)
    h = _device_handle(DDparam, A)
    lib = D.load_library()
    val = D._f32 if DDparam.is_single else D._f64
    D._check(lib, getattr(lib, "mg_dd_apply_" + sfx)(h, val(bb), val(x), A.shape[0], int(niter), int(doTranspose)),
             "mg_dd_apply_" + sfx)
    return x, DDparam


def getDDpreconditioner(A, DDparam: DomainDecompositionParam, B, doTranspose: int = 0):
    """r -> one sweep from x = 0 (DomainDecomposition.jl:136-146); the closure reuses its buffers, as the reference does.
    Usable as ``M`` of scipy's gmres (wrapped in a LinearOperator).  It is the reference's mixed closure: x0 and rt in VAL, x_new
    in eltype(B) - a complex128 ``B`` with a ComplexF32 DDparam narrows r and widens the result, so a single sweep preconditions a
    ComplexF64 Krylov method."""
    VAL = np.dtype(DDparam.VAL)
    x0 = np.zeros(np.shape(B), dtype=VAL)
    x_new = np.zeros(np.shape(B), dtype=np.asarray(B).dtype if np.asarray(B).dtype.kind in "fc" else VAL)
    rt = np.zeros(np.shape(B), dtype=VAL)

    def Prec(r):
        x0[...] = 0.0
        rt[...] = np.reshape(r, rt.shape)
        x_new[...] = solveDDSerial(A, rt, x0, DDparam, 1, doTranspose)[0]
        return x_new

    return Prec
