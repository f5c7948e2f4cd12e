"""Geometric multigrid setup on the host (CPU), feeding the device cycle library.

Mirrors reference src/Multigrid/MGsetup.jl: ``MGsetup`` (l.7-138), ``getRelaxPrec`` (l.142-160),
``adjustMemoryForNumRHS`` (l.166-223), ``replaceMatrixInHierarchy`` (l.226-270),
``transposeHierarchy`` (l.274-318; ``adjointHierarchy``: the same lines for complex VAL), ``defineCoarsestAinv`` (l.323-355), ``getSPAIprec`` (l.359-362).

The hierarchy is built on the CPU "exactly as the reference does" (BASELINE.json north_star); the
cycle itself never runs here - it is owned by the HIP library (``device.py``).
"""
from __future__ import annotations

import time

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from .mgdef import MGparam, destroyCoarsestLU, _release_device, factor_val, factor_vals, is_complex, is_single
from .transfer_operators import getFWInterp


class multilevelOperatorConstructor:
    """Mirror of MGdef.jl:31-46: rediscretisation on every level instead of Galerkin."""

    def __init__(self, param, getOperator, restrictParams):
        self.param = param
        self.getOperator = getOperator
        self.restrictParams = restrictParams


def getMultilevelOperatorConstructor(param, getOperator, restrictParams):
    if restrictParams is None or (isinstance(restrictParams, (list, tuple)) and len(restrictParams) == 0):
        return multilevelOperatorConstructor(None, lambda mesh, p: getOperator(mesh),
                                             lambda mf, mc, p, level: None)
    return multilevelOperatorConstructor(param, getOperator, restrictParams)


def _as_csr(A):
    dt = np.dtype(A.dtype)
    if dt != np.complex64:                                           # (a ComplexF32 hierarchy keeps its single operators)
        dt = np.complex128 if np.iscomplexobj(A.data if sp.issparse(A) else A) else np.float64
    A = sp.csr_matrix(A, dtype=dt)
    A.sort_indices()
    return A


def getSPAIprec(A):
    """Q_i = conj(diag)_i / s_i with s_i = sum_j |AT[i,j]|^2 (MGsetup.jl:359-362).

    Row i of the reference's AT is COLUMN i of A, so s is the column-wise sum of squares of A
    (equal to the row norm only for symmetric A).
    """
    A = _as_csr(A)
    if np.iscomplexobj(A.data):
        # complex VAL: Q = conj(AT[i,i]) / sum_j |AT[i,j]|^2 of the reference's AT = A^H (MGsetup.jl:359-362, real^2 + imag^2):
        # the diagonal of AT is conj(diag(A)), its row i is column i of A conjugated.  (Applied as x += d.*r through A's
        # own diagonal, d = omega * conj(diag(A)) / colsumsq|A| - the conj of getRelaxPrec's conj(relaxParam*Q), l.148-149.)
        s = np.bincount(A.indices, weights=A.data.real ** 2 + A.data.imag ** 2, minlength=A.shape[1])
        return np.conj(A.diagonal()) / s
    from .hostlib import col_sumsq
    s = col_sumsq(A)                                # (thread-parallel on the host; the scipy / numpy line below otherwise)
    if s is None:
        s = np.bincount(A.indices, weights=A.data * A.data, minlength=A.shape[1])
    return A.diagonal() / s


def getRelaxPrec(A, relaxType: str, relaxParam=1.0, Mesh_l=None, withCellsBlock: bool = False, device: bool = False):
    """Jac: d = omega/diag (MGsetup.jl:145-147).  SPAI: d = omega*diag/colnorm^2 (l.148-149).  The Vanka types: the cells'
    blocks of setupVankaFacesPreconditioner on the level's mesh (l.153-154; relaxParam a float or a tuple of two).

    Complex A (the applied operator, = the reference's AT^H): the reference's d = conj(relaxParam ./ diag(AT)) and
    conj(relaxParam*getSPAIprec(AT)) become d = omega/diag(A) and d = omega*conj(diag(A))/colsumsq|A| - for a real A both
    are the formulas above.

    ``device=True`` (the Vanka types only; a param with ``vankaDeviceSetup=True``): the blocks are built on the device
    (``setupVankaFacesPreconditioner(..., device=True)``) and returned as the same host array."""
    from .vanka import getVankaRelaxType, setupVankaFacesPreconditioner
    isVanka, VankaType = getVankaRelaxType(relaxType)
    if isVanka:
        if Mesh_l is None:
            raise ValueError(f"relaxType={relaxType!r} needs the level's mesh (getRelaxPrec(A, relaxType, relaxParam, Mesh_l, withCellsBlock))")
        if device:
            return setupVankaFacesPreconditioner(A, Mesh_l, relaxParam, withCellsBlock, VankaType, device=True)
        return setupVankaFacesPreconditioner(A, Mesh_l, relaxParam, withCellsBlock, VankaType)
    if relaxType == "hybridVankaFacesKaczmarz":
        raise NotImplementedError("RelaxHybridVanka / getHybridVankaFaces are out of scope (the cycle's call is commented out in the reference)")
    if np.iscomplexobj(A.data if sp.issparse(A) else A):
        A = _as_csr(A)
        # A complex64 operator (a ComplexF32 hierarchy, whose As are converted first: MGsetup.jl:31-33) gives complex64 relaxPrecs:
        # the formulas are evaluated in double on the single values and the result is converted once, as the reference's
        # convert(Array{VAL}, conj(relaxParam ./ diag(AT))) does with its Float64 relaxParam (MGsetup.jl:145-149).
        cdt = np.complex64 if A.dtype == np.complex64 else np.complex128
        A = A.astype(np.complex128)
        if relaxType in ("Jac", "Jac-GMRES"):
            return np.ascontiguousarray(float(relaxParam) / A.diagonal(), dtype=cdt)
        if relaxType == "SPAI":
            return np.ascontiguousarray(float(relaxParam) * getSPAIprec(A), dtype=cdt)
        raise ValueError("Unknown relaxation type !!!!")
    if relaxType in ("Jac", "Jac-GMRES"):
        return np.ascontiguousarray(float(relaxParam) / _as_csr(A).diagonal(), dtype=np.float64)
    if relaxType == "SPAI":
        return np.ascontiguousarray(float(relaxParam) * getSPAIprec(A), dtype=np.float64)
    raise ValueError("Unknown relaxation type !!!!")


def _is_vanka(param: MGparam) -> bool:
    from .vanka import getVankaRelaxType
    return getVankaRelaxType(param.relaxType)[0]


def _vanka_device_kw(param: MGparam) -> dict:
    """getRelaxPrec's ``device=True`` for a param that asked for the device set-up of its Vanka blocks (``vankaDeviceSetup``)."""
    return {"device": True} if getattr(param, "vankaDeviceSetup", False) and _is_vanka(param) else {}


def _relax_param_arr(param: MGparam):
    rp = param.relaxParam
    if _is_vanka(param) and isinstance(rp, tuple) and len(rp) == 2 and all(np.isscalar(w) for w in rp):
        return [rp] * param.levels      # one (w1, w2) pair, not an Array: copied to every level (MGsetup.jl:15-19)
    # (any other sequence holds one entry per level, each a float or a (w1, w2) pair)
    if isinstance(param.relaxParam, (list, tuple, np.ndarray)):
        return list(param.relaxParam)
    return [param.relaxParam] * param.levels


def galerkin(R, A, P):
    """A_c = R*(A*P): the CSR view of ``Act = Ps[l]*AT*Rs[l]`` evaluated left to right (MGsetup.jl:102).
    The reference's serial Julia SpGEMM is the bulk of its setup time; here it is row-parallel on the host
    (csrc/mg_host.cpp) - still CPU, still before the device ever sees the hierarchy."""
    if np.iscomplexobj(A.data):    # complex VAL: scipy's SpGEMM (real P, R; host setup speed is not a goal here)
        Ac = (R @ (A @ P)).tocsr()   # (complex64 A with float32 P, R: the product is formed and kept in single, MGsetup.jl:108-110)
        Ac.sort_indices()
        return Ac
    from .hostlib import galerkin_dense_gpu, galerkin_dense_gpu_ok, galerkin_sparse_gpu, galerkin_sparse_gpu_ok, spgemm
    # (opt-in, MG_SETUP_GPU=1: the largest products of an SA-AMG setup on the GPU - same pattern, values to rounding; hostlib.py)
    if galerkin_dense_gpu_ok(A, P):        # nearly dense levels: dense GEMMs
        Ac = galerkin_dense_gpu(R, A, P)
        if Ac is not None:
            return Ac
    if galerkin_sparse_gpu_ok(A, P):       # 10^10 products and more: rocSPARSE's SpGEMM
        Ac = galerkin_sparse_gpu(R, A, P)
        if Ac is not None:
            return Ac
    return spgemm(R, spgemm(A, P))


def defineCoarsestAinv(param: MGparam, Ac) -> None:
    """Coarsest-level factorisation (MGsetup.jl:323-355).  Default branch: ``lu(sparse(AT'))`` (l.350).  A solver object
    preset in ``param.LU`` is set up on the coarsest matrix and stays the object the caller put there (l.323-331)."""
    from .mgdef import _solver_object
    kind = _solver_object(param.LU)
    if kind == "dd":                              # LU.Mesh = Meshes[end]; setupDDSerial(AT, LU)
        from .domain_decomposition import setupDDSerial
        LU = param.LU
        if not param.Meshes:
            raise ValueError("a DomainDecompositionParam as coarsest solver needs the coarsest mesh: the hierarchy has none (SA-AMG)")
        # (a ComplexF32 hierarchy takes a ComplexF32 sweep - getDomainDecompositionParam(np.complex64, ..., singleValues=True) - set up
        # on its complex64 coarsest operator; a ComplexF64 one stays unserved there)
        if is_single(param) and np.dtype(LU.VAL) != np.complex64:
            raise NotImplementedError("a Schwarz coarsest solve is not served for ComplexF32 hierarchies (singlePrecision=True)")
        if np.dtype(LU.VAL) != np.dtype(param.VAL):
            raise TypeError("param.LU is a DomainDecompositionParam of %s, the hierarchy of %s" % (np.dtype(LU.VAL), np.dtype(param.VAL)))
        LU.Mesh = param.Meshes[-1]
        setupDDSerial(_as_csr(Ac), LU)            # (closes LU's device handle first: a resident hierarchy that borrows it gives it back)
        return
    if kind == "pjs":                             # setupSolver(sparse(AT'), LU)
        from .parallel_julia_solver import setupLUFactor
        if np.dtype(param.LU.VAL) not in factor_vals(param):
            raise TypeError("param.LU is a parallelJuliaSolver of %s, the hierarchy of %s" % (np.dtype(param.LU.VAL), np.dtype(param.VAL)))
        # (a single solver object factorises the widened matrix in double itself and keeps single factors)
        setupLUFactor(_as_csr(Ac).astype(factor_val(param)), param.LU, upload=False)
        return
    if param.coarseSolveType == "MUMPS":
        raise NotImplementedError("MUMPS coarse solve is dead code in the reference (Multigrid.jl:29-40)")
    if param.coarseSolveType == "GMRES":
        # Jacobi-preconditioned FGMRES coarse solve (MGcycle.jl:152-168): param.LU = relaxParam ./ diag(AT) (l.334),
        # which only broadcasts for a scalar relaxParam
        if isinstance(param.relaxParam, (list, tuple, np.ndarray)):
            raise ValueError("coarseSolveType='GMRES' needs a scalar relaxParam (MGsetup.jl:334 broadcasts it over diag(AT))")
        Acs = _as_csr(Ac)
        param.LU = np.ascontiguousarray(float(param.relaxParam) / Acs.diagonal(), dtype=Acs.dtype)
        return
    # (a ComplexF32 hierarchy factorises its single coarsest operator in double: UMFPACK has no single form, MGsetup.jl:350)
    param.LU = coarse_lu(sp.csr_matrix(Ac).astype(np.complex128) if is_single(param) else Ac)


def coarse_lu(Ac):
    """``lu(sparse(AT'))`` (MGsetup.jl:350).  Julia's lu is UMFPACK, which orders symmetric-pattern matrices by AMD on
    A+A'; SuperLU's closest ordering is MMD on A'+A (half the fill of its COLAMD default on these operators: 18M vs
    40M nonzeros per factor on a 33^3 27-point level)."""
    return spla.splu(sp.csc_matrix(Ac), permc_spec="MMD_AT_PLUS_A")


def _of_val(param: MGparam, A):
    """The operator in param.VAL: a complex hierarchy holds every A as complex128 (a real fine operator included); a complex
    operator needs VAL = ComplexF64."""
    A = _as_csr(A)
    if is_single(param):               # MGsetup.jl:31-33: As converted to VAL
        return A.astype(np.complex64)
    if is_complex(param):
        return A.astype(np.complex128)
    if np.iscomplexobj(A.data):
        raise TypeError("complex operator with VAL=Float64: use getMGparam(VAL=np.complex128)")
    return A


def MGsetup(ATf, Mesh, param: MGparam, nrhs: int = 1, verbose: bool = False) -> MGparam:
    """Build As/Ps/Rs/relaxPrecs level by level (MGsetup.jl:7-138).

    ``ATf`` is either the fine operator A (any scipy sparse; held as CSR = the reference's transposed CSC)
    or a ``multilevelOperatorConstructor`` (rediscretisation; then ``geometric=True``, l.53).
    """
    systems = param.transferOperatorType in ("SystemsFacesLinear", "SystemsFacesMixedLinear")
    withCellsBlock = param.transferOperatorType == "SystemsFacesMixedLinear"
    if param.transferOperatorType != "FullWeighting" and not systems:
        raise NotImplementedError("transferOperatorType is 'FullWeighting', 'SystemsFacesLinear' or 'SystemsFacesMixedLinear'")
    if param.coarseSolveType == "VankaFaces":
        raise NotImplementedError("coarseSolveType='VankaFaces' calls functions that are commented out in the reference")
    if _is_vanka(param) and is_complex(param):
        if not param.complexVanka:
            raise NotImplementedError("Vanka hierarchies serve VAL=Float64 (the stand-alone RelaxVankaFacesColor takes complex operators); "
                                      "a complex one is asked for with getMGparam(np.complex128, ..., complexVanka=True)")
        if not systems:
            raise NotImplementedError("a complex Vanka hierarchy needs transferOperatorType 'SystemsFacesLinear' or 'SystemsFacesMixedLinear'")
    _release_device(param)
    levels = param.levels
    relaxParamArr = _relax_param_arr(param)
    geometric = isinstance(ATf, multilevelOperatorConstructor)
    PDEparam = None
    if geometric:
        As = [_of_val(param, ATf.getOperator(Mesh, ATf.param))]
        PDEparam = ATf.param
    else:
        As = [_of_val(param, ATf)]
    if systems:
        from .vanka import getVankaBlockSize
        N = int(getVankaBlockSize(Mesh.n, withCellsBlock)[1].sum()) + (int(np.prod(Mesh.n)) if withCellsBlock else 0)
        if As[0].shape[0] != N:
            raise NotImplementedError(f"transferOperatorType={param.transferOperatorType!r} serves staggered-grid operators: a mesh of "
                                      f"{list(map(int, Mesh.n))} cells has {N} face{' and cell' if withCellsBlock else ''} unknowns, "
                                      f"the operator has {As[0].shape[0]} rows")
    from .operators import getRegularMesh
    Meshes = [Mesh]
    Ps, Rs, relaxPrecs = [], [], []
    n = np.asarray(Mesh.n, dtype=np.int64)
    Cop = As[0].nnz
    for l in range(1, levels):                      # l is the reference's 1-based level
        t0 = time.perf_counter()
        A = As[l - 1]
        if systems:                                         # MGsetup.jl:63-73
            from .systems import getLinearOperatorsSystemsFaces
            P, R, nc = getLinearOperatorsSystemsFaces(n, withCellsBlock)
            R = (R * (0.5 ** Meshes[l - 1].dim)).tocsr()
        else:
            P, nc_nodes = getFWInterp(n + 1, geometric)
            nc = nc_nodes - 1
            R = (P.T * (0.5 ** Meshes[l - 1].dim)).tocsr()      # RT = P*0.5^dim always (MGsetup.jl:56-60)
        R.sort_indices()
        if is_single(param):                                    # Ps / Rs in real(VAL) (MGsetup.jl:79-82)
            P, R = P.astype(np.float32), R.astype(np.float32)
        relaxPrecs.append(getRelaxPrec(A, param.relaxType, relaxParamArr[l - 1], Meshes[l - 1], withCellsBlock,
                                       **_vanka_device_kw(param)))
        if P.shape[0] == P.shape[1]:
            if verbose:
                print(f"Stopped Coarsening at level {l}")
            param.levels = l                                  # MGsetup.jl:84-92
            break
        Ps.append(P)
        Rs.append(R)
        Meshes.append(getRegularMesh(Meshes[l - 1].domain, nc))
        if geometric:
            PDEparam = ATf.restrictParams(Meshes[l - 1], Meshes[l], PDEparam, l)
            Ac = _of_val(param, ATf.getOperator(Meshes[l], PDEparam))
        else:
            Ac = galerkin(R, A, P)
        As.append(Ac)
        Cop += Ac.nnz
        if verbose:
            print(f"MG setup: {n} cells took:{time.perf_counter() - t0:.3f}")
        n = nc
    if verbose:
        print("MG setup: Operator complexity = ", Cop / As[0].nnz)
    param.As = As
    param.Meshes = Meshes
    defineCoarsestAinv(param, As[-1])
    param.Ps = Ps
    param.Rs = Rs
    param.relaxPrecs = relaxPrecs
    adjustMemoryForNumRHS(param, nrhs, verbose)
    param.doTranspose = 0
    return param


def adjustMemoryForNumRHS(param: MGparam, nrhs: int = 1, verbose: bool = False) -> MGparam:
    """Size the per-level b/r/x scratch for ``nrhs`` columns (MGsetup.jl:166-223).

    On the device the scratch lives in HBM; this records the width and, when a handle exists,
    re-sizes it (``mg_set_nrhs``) only if the width changed, as the reference does (l.171-188).
    """
    if len(param.As) == 0:
        raise RuntimeError("The Hierarchy is empty - run a setup first.")
    nrhs = int(nrhs)
    if nrhs < 1:
        raise ValueError("nrhs must be >= 1")
    if param.nrhs != nrhs:
        param.nrhs = nrhs
        if param.device is not None:
            param.device.set_nrhs(nrhs)
    return param


def replaceMatrixInHierarchy(param: MGparam, A, verbose: bool = False) -> None:
    """New fine matrix, same P/R: recompute relaxPrecs, Galerkin products and the coarse LU (MGsetup.jl:226-270).  On a resident
    param with ``coarseDeviceInverse=True`` the explicit inverse of the new coarsest operator is rebuilt in HBM (mg_rap_*); the
    host still factors it (``param.LU``) and uploads nothing.  A resident ComplexF32 param takes the device path where it carries
    ``singleDeviceSetup=True`` (mg_rap_CF32) and the host path with a fresh upload otherwise; with ``singleKcycle=True`` the ComplexF64
    rule holds: K with Jac / SPAI keeps the handle, Jac-GMRES takes the host path."""
    relaxParamArr = _relax_param_arr(param)
    A = _of_val(param, A)
    # (a ComplexF32 hierarchy is recomputed on the host and uploaded again, unless its param asked for the device re-setup:
    #  singleDeviceSetup, mg_rap_CF32)
    served = not is_single(param) or bool(getattr(param, "singleDeviceSetup", False))
    on_device = param.device is not None and param.relaxType in ("Jac", "Jac-GMRES", "SPAI") and served
    if param.device is not None and served and is_complex(param) and _is_vanka(param) and getattr(param, "vankaDeviceSetup", False):
        on_device = True       # (mg_rap_CF64 / _CF32 with the option vanka_device_setup: operators and blocks recomputed in HBM)
    if on_device and is_complex(param):
        # (mg_rap_CF64.  A Schwarz coarsest solver borrows a device handle of its own, set up on the coarsest matrix: host path)
        from .mgdef import _solver_object
        on_device = param.relaxType != "Jac-GMRES" and _solver_object(param.LU) != "dd"
    if on_device:
        old = param.As[0]
        same = (A.shape == old.shape and A.nnz == old.nnz and np.array_equal(A.indptr, old.indptr)
                and np.array_equal(A.indices, old.indices))
        if same:
            from .device import MGDeviceError
            try:   # numeric-only Galerkin products on the device (fixed P, R and patterns: SURVEY 8f-2)
                param.device.replace_matrix(param, A)
                param.doTranspose = 0
                return
            except MGDeviceError:
                pass   # e.g. SA-AMG rows beyond the kernel's cap: the host path below applies
    param.As[0] = A
    for l in range(1, param.levels):
        Al = param.As[l - 1]
        Mesh_l = param.Meshes[l - 1] if param.Meshes else None      # MGsetup.jl:247-252
        param.relaxPrecs[l - 1] = getRelaxPrec(Al, param.relaxType, relaxParamArr[l - 1], Mesh_l,
                                               param.transferOperatorType == "SystemsFacesMixedLinear", **_vanka_device_kw(param))
        param.As[l] = galerkin(param.Rs[l - 1], Al, param.Ps[l - 1])
    defineCoarsestAinv(param, param.As[-1])
    param.doTranspose = 0
    _release_device(param)            # re-uploaded lazily on the next cycle


def transposeHierarchy(param: MGparam, verbose: bool = False) -> None:
    """Transpose every operator, swap P<->R roles (MGsetup.jl:274-318).  Real VAL: conj is a no-op."""
    if is_complex(param):
        raise NotImplementedError("transposeHierarchy of a ComplexF64 / ComplexF32 hierarchy (the device transpose serves FP64 handles)")
    if _is_vanka(param):
        raise NotImplementedError("transposeHierarchy of a Vanka hierarchy (the reference refuses it too: MGsetup.jl:288-292)")
    if param.relaxType not in ("Jac", "Jac-GMRES", "SPAI"):
        raise RuntimeError("Not supported")
    param.As[0] = _as_csr(param.As[0].T)
    param.doTranspose = (param.doTranspose + 1) % 2
    for l in range(1, param.levels):
        # reference: Ps[l] = sparse(Rs[l]'); Rs[l] = sparse(Ps[l]')  (the second line reads the NEW Ps[l],
        # l.298-299, so both end up holding the old R): reproduced literally.
        newP = _as_csr(param.Rs[l - 1].T)
        param.Ps[l - 1] = newP
        param.Rs[l - 1] = _as_csr(newP.T)
        param.As[l] = _as_csr(param.As[l].T)
    destroyCoarsestLU(param)
    param.LU = None        # MGsetup.jl:310-311 factors the transposed coarsest matrix itself: a solver object is replaced
    defineCoarsestAinv(param, param.As[-1])
    # The resident hierarchy is transposed in HBM (mg_transpose_hierarchy: counting-sort CSR transposes, dense coarsest inverse
    # transposed in place, device formats rebuilt) instead of being dropped and uploaded again; what the library cannot do there
    # (sparse coarsest factors) falls back to the lazy re-upload.
    if param.device is not None:
        from .device import MGDeviceError
        try:
            param.device.transpose_hierarchy()
        except MGDeviceError:
            _release_device(param)


def _adjoint_csr(M):
    """``sparse(M')`` as this package holds operators: CSR of conj(M)^T with sorted indices, M's dtype kept."""
    T = sp.csr_matrix(M.conj().T, dtype=M.dtype)
    T.sort_indices()
    return T


def adjointHierarchy(param: MGparam, verbose: bool = False) -> None:
    """``transposeHierarchy`` (MGsetup.jl:274-318) for complex VAL, where ``'`` is the adjoint: As[l] <- As[l]' (the conjugate
    transpose) on every level, relaxPrecs[l] <- conj(relaxPrecs[l]), Ps[l] <- Rs[l]', Rs[l] <- (new Ps[l])' (Rs keeps its values: the
    reference's literal pair of assignments), doTranspose flipped.  Coarsest solve: ``param.LU <- conj(param.LU)`` for
    coarseSolveType "GMRES" (l.304-305), else the factorisation of the new As[end] (a preset solver object is replaced, as
    ``transposeHierarchy`` does it).  Serves ComplexF64 params and ``singlePrecision`` ones (dtypes kept); a real param is
    ``transposeHierarchy``'s.  A resident hierarchy is flipped in HBM (mg_adjoint_hierarchy_CF64 / _CF32); what the library refuses
    there (sparse coarsest factors, a Schwarz coarsest solve) falls back to the lazy re-upload, and so does a ``singleKcycle`` param
    (flipping its resident hierarchy in HBM is not built)."""
    if not is_complex(param):
        raise TypeError("adjointHierarchy serves complex params (VAL=ComplexF64, singlePrecision or not): a real hierarchy is "
                        "flipped by transposeHierarchy")
    if _is_vanka(param):
        raise NotImplementedError("adjointHierarchy of a Vanka hierarchy (the reference refuses it too: MGsetup.jl:288-292)")
    if param.relaxType not in ("Jac", "Jac-GMRES", "SPAI"):
        raise RuntimeError("Not supported")
    if len(param.As) == 0:
        raise RuntimeError("The Hierarchy is empty - run a setup first.")
    param.As[0] = _adjoint_csr(param.As[0])
    param.doTranspose = (param.doTranspose + 1) % 2
    for l in range(1, param.levels):
        if verbose:
            print("MG transpose level: ", l)
        param.relaxPrecs[l - 1] = np.conj(param.relaxPrecs[l - 1])
        newP = _adjoint_csr(param.Rs[l - 1])              # (real: the transpose, float32 kept for a single hierarchy)
        param.Ps[l - 1] = newP
        param.Rs[l - 1] = _adjoint_csr(newP)
        param.As[l] = _adjoint_csr(param.As[l])
    if param.coarseSolveType == "GMRES" and isinstance(param.LU, np.ndarray):
        param.LU = np.conj(param.LU)                      # MGsetup.jl:304-305
    else:
        destroyCoarsestLU(param)
        param.LU = None        # MGsetup.jl:310-311 factors the adjoint coarsest matrix itself: a solver object is replaced
        defineCoarsestAinv(param, param.As[-1])
    if param.device is not None and is_single(param) and getattr(param, "singleKcycle", False):
        _release_device(param)     # (a singleKcycle hierarchy is not flipped in HBM: uploaded again by the next cycle)
    if param.device is not None:
        from .device import MGDeviceError
        try:
            param.device.adjoint_hierarchy(param)
        except MGDeviceError:
            _release_device(param)
