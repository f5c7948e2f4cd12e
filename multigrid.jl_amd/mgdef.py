"""Hierarchy container and constructors (host side).

Mirrors reference src/Multigrid/MGdef.jl: ``MGparam`` (l.91-116), ``getMGparam`` (l.149-161),
``clear!`` (l.179-189), ``destroyCoarsestLU`` (l.191-206), ``hierarchyExists`` (l.208),
``copySolver`` (l.138-145).

Storage convention.  The reference keeps every operator transposed as a ``SparseMatrixCSC``
so that ``A*x`` is ``AT'*x`` (MGdef.jl:75-77): CSC of A' *is* CSR of A.  Here the same arrays are held
as scipy CSR matrices named for what they apply:

    reference ``As[l]``  (AT, CSC)            <->  ``As[l]``  CSR of A_l            (n_l  x n_l)
    reference ``Ps[l]``  (PT, CSC n_c x n_f)  <->  ``Ps[l]``  CSR of P_l            (n_f  x n_c)
    reference ``Rs[l]``  (RT, CSC n_f x n_c)  <->  ``Rs[l]``  CSR of R_l            (n_c  x n_f)

so ``X.indptr`` is Julia's ``colptr-1`` and ``X.indices`` is ``rowval-1``.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Callable, List, Optional

import numpy as np


@dataclass
class MGparam:
    levels: int = 3
    numCores: int = 8
    maxOuterIter: int = 20
    relativeTol: float = 1e-6
    relaxType: str = "SPAI"
    relaxParam: Any = 1.0
    relaxPre: Callable[[int], int] = None
    relaxPost: Callable[[int], int] = None
    cycleType: str = "V"
    Ps: List[Any] = field(default_factory=list)
    Rs: List[Any] = field(default_factory=list)
    As: List[Any] = field(default_factory=list)
    relaxPrecs: List[Any] = field(default_factory=list)
    nrhs: int = 0                      # what memCycle is sized for (adjustMemoryForNumRHS)
    coarseSolveType: str = "NoMUMPS"
    LU: Any = None
    doTranspose: int = 0
    strongConnParam: float = 0.4
    FilteringParam: float = 0.0
    Meshes: List[Any] = field(default_factory=list)
    transferOperatorType: str = "FullWeighting"
    singlePrecision: bool = False
    blockCoarseGMRES: bool = False     # coarseSolveType "GMRES" on a complex hierarchy: serve blocks by the block GMRES coarsest solve
    complexVanka: bool = False         # a Vanka relaxType on a complex hierarchy: the cell-block smoother in the complex cycle
    vankaBlocks: bool = False          # complexVanka only: serve blocks of right-hand sides by the block form of the smoother
    vankaDeviceSetup: bool = False     # complexVanka only: the cells' blocks are built (and, ComplexF64 or singleDeviceSetup, refreshed) on the device
    coarseDeviceInverse: bool = False  # the coarsest operator's explicit inverse is built (and refreshed) on the device
    singleDeviceSetup: bool = False    # singlePrecision only: replaceMatrixInHierarchy refreshes the resident hierarchy in HBM
    singleKcycle: bool = False         # singlePrecision only: the K-cycle and Jac-GMRES smoothing on the ComplexF32 hierarchy
    blockKcycle: bool = False          # complex only: blocks on a K-cycle / Jac-GMRES hierarchy, the block one long vector (columns coupled)
    VAL: Any = np.float64
    IND: Any = np.int64
    # device side (no reference counterpart): handle of the HIP cycle library + last residual history
    device: Any = None
    resvec: Optional[np.ndarray] = None
    flag: int = 0


def getMGparam(VAL=np.float64, IND=np.int64, levels=3, numCores=8, maxIter=20, relativeTol=1e-6,
               relaxType="SPAI", relaxParam=1.0, relaxPre=2, relaxPost=2, cycleType="V",
               coarseSolveType="NoMUMPS", strongConnParam=0.4, FilteringParam=0.0,
               transferOperatorType="FullWeighting", *, singlePrecision: bool = False,
               blockCoarseGMRES: bool = False, complexVanka: bool = False, vankaBlocks: bool = False,
               vankaDeviceSetup: bool = False, coarseDeviceInverse: bool = False,
               singleDeviceSetup: bool = False, singleKcycle: bool = False,
               blockKcycle: bool = False) -> MGparam:
    """Positional constructor with the reference's defaults (MGdef.jl:149-161).

    ``relaxPre``/``relaxPost`` may be ints or functions of the (1-based) level, as in MGdef.jl:98-99,158-159.
    ``VAL`` is ``Float64`` or ``ComplexF64`` (np.complex128: the _CF64 entry points, single GPU, V/W/F cycles, Jac/SPAI);
    every other value type is refused.  ``singlePrecision=True`` (keyword only) with ``np.complex128`` gives the reference's
    VAL = ComplexF32 hierarchy (``param.VAL = np.complex64``, ``param.singlePrecision = True``, MGdef.jl:151): operators,
    relaxPrecs and cycle in single precision (the _CF32 entry points), coarsest factorisation in double, and the ComplexF64
    Krylov drivers preconditioned by the single cycle (the mixed branch of getMultigridPreconditioner).
    ``blockCoarseGMRES=True`` (keyword only) with a complex ``VAL`` and ``coarseSolveType="GMRES"`` switches on the block form of
    that coarsest solve (the reference's blockFGMRES branch, MGcycle.jl:165-167): blocks of 2 to 16 right-hand sides are then
    served on the hierarchy; without it they are refused.  The columns of a block are coupled by that solve.
    ``complexVanka=True`` (keyword only) with a complex ``VAL`` and a Vanka ``relaxType`` (VankaFaces, EconVankaFaces, VankaFacesAdd)
    lets ``MGsetup`` build the complex Vanka hierarchy of the reference (Systems transfers, complex64 blocks per level) and the
    device run it: ComplexF64 with cycles V / W / F / K, ``singlePrecision`` with V / W / F (K with ``singleKcycle=True``), one
    right-hand side.  Without it a
    complex Vanka param is refused by ``MGsetup``, as before.
    ``vankaBlocks=True`` (keyword only, with ``complexVanka=True``) switches on the block form of that smoother: blocks of up to 16
    right-hand sides are then served on the hierarchy for the cycles V / W / F (solveMG, recursiveCycle, getMultigridPreconditioner,
    the block _CFP64 drivers, the device's ``block_*`` methods); without it they are refused, as before.
    ``vankaDeviceSetup=True`` (keyword only, with ``complexVanka=True``; with or without ``singlePrecision`` and ``vankaBlocks``)
    builds the cells' blocks on the device: ``MGsetup`` and the host path of ``replaceMatrixInHierarchy`` take ``relaxPrecs[l]`` from
    ``setupVankaFacesPreconditioner(..., device=True)`` (ordinary host arrays, as before), the upload builds every level's blocks in
    HBM from the resident operator instead of sending them, and ``replaceMatrixInHierarchy`` of a resident ComplexF64 param with
    an unchanged pattern recomputes operators and blocks in HBM and keeps the handle.  Without it nothing changes.
    ``coarseDeviceInverse=True`` (keyword only; Float64 and ComplexF64, with or without ``singlePrecision``) builds the explicit
    inverse of the coarsest operator on the device, from the operator resident there (a dense inverse with partial pivoting,
    ``mg_build_coarse_dense_inverse_*``), instead of ``LU.solve(eye)`` on the host plus an upload; ``replaceMatrixInHierarchy`` of a
    resident param then rebuilds it in HBM behind the Galerkin products.  ``param.LU`` stays the host's factorisation.  The flag
    is a no-op where the coarsest solve is not a dense inverse of at most ``coarse_device_inverse_max`` (8192) rows: a solver
    object in ``param.LU`` (Schwarz, parallelJuliaSolver) or a larger coarsest level take today's route.  With
    ``coarseSolveType="GMRES"`` it is refused (there is no inverse to build).  Without it nothing changes.
    ``singleDeviceSetup=True`` (keyword only, with ``singlePrecision=True``) lets ``replaceMatrixInHierarchy`` of a resident
    ComplexF32 param with an unchanged pattern recompute the Galerkin products and relaxPrecs in HBM (``mg_rap_CF32``: single
    values widened on load, ComplexF64 sums, one rounding on the store) and keep the handle, under the conditions of the
    ComplexF64 path: Jac or SPAI, or a Vanka hierarchy with ``vankaDeviceSetup=True``; the GMRES coarsest solve and
    ``coarseDeviceInverse`` are refreshed there too.  Without it a ComplexF32 param is recomputed on the host and uploaded again,
    as before.
    ``singleKcycle=True`` (keyword only, with ``singlePrecision=True``) serves ``cycleType="K"`` and ``relaxType="Jac-GMRES"`` on the
    ComplexF32 hierarchy (the handle's option ``single_kcycle``, ``mg_set_schedule_CF32``): V / W / F / K with Jac / SPAI /
    Jac-GMRES, and K with the Vanka smoothers, one right-hand side.  The directions Z and A Z are complex64 and the product is formed
    in single; the Gram sums, the small least squares and the break test are formed in double (a deviation from the reference, which
    forms them in ComplexF32 where the residual estimate is noise at the 1e-5 break).  Blocks of right-hand sides stay refused on
    such a schedule (unless ``blockKcycle=True`` is set as well).  Without it a ComplexF32 param with ``"K"`` or ``"Jac-GMRES"`` is
    refused, as before.
    ``blockKcycle=True`` (keyword only, with a complex ``VAL``; the handle's option ``kcycle_blocks``) serves blocks of 1 to 16
    right-hand sides on a hierarchy with ``cycleType="K"`` and / or ``relaxType="Jac-GMRES"`` in the reference's form: every FGMRES
    relaxation and every K step takes the block as ONE long vector of length n*k (FGMRES.jl:51-53), with one H, one t and one break
    test for the whole block.  The columns of a block are therefore coupled - a column's result depends on its neighbours and on
    their scaling, and differs from what the same column gives alone.  A Jac-GMRES cycle is non-linear in its right-hand side:
    as a preconditioner it belongs under block FGMRES (``solveBlockGMRES_MG_CFP64``), not block BiCGSTAB.  With ``singlePrecision``
    it needs ``singleKcycle=True`` as well, with ``coarseSolveType="GMRES"`` ``blockCoarseGMRES=True``.  Vanka with ``"K"`` and a
    Schwarz coarsest solve stay refused on a block.  Without it such blocks are refused, as before; a real ``VAL`` refuses it.
    """
    if np.dtype(VAL) not in (np.dtype(np.float64), np.dtype(np.complex128)):
        raise TypeError("only VAL=Float64 or VAL=ComplexF64 (np.complex128) is supported on the device path; a ComplexF32 "
                        "hierarchy is getMGparam(np.complex128, ..., singlePrecision=True)")
    if singlePrecision and np.dtype(VAL) != np.complex128:
        raise NotImplementedError("singlePrecision=True serves VAL=ComplexF64 (Float32 real hierarchies are out of scope)")
    if blockCoarseGMRES and (np.dtype(VAL) != np.complex128 or str(coarseSolveType) != "GMRES"):
        raise NotImplementedError("blockCoarseGMRES=True serves VAL=ComplexF64 (singlePrecision or not) with coarseSolveType='GMRES'")
    if complexVanka:
        from .vanka import getVankaRelaxType
        if np.dtype(VAL) != np.complex128 or not getVankaRelaxType(str(relaxType))[0]:
            raise NotImplementedError("complexVanka=True serves VAL=ComplexF64 (singlePrecision or not) with a Vanka relaxType")
    if vankaBlocks and not complexVanka:
        raise NotImplementedError("vankaBlocks=True serves a complex Vanka hierarchy (complexVanka=True)")
    if vankaDeviceSetup and not complexVanka:
        raise NotImplementedError("vankaDeviceSetup=True serves a complex Vanka hierarchy (complexVanka=True); FP64 Vanka hierarchies "
                                  "set their blocks up on the host")
    if coarseDeviceInverse and str(coarseSolveType) == "GMRES":
        raise NotImplementedError("coarseDeviceInverse=True builds the coarsest operator's explicit inverse: coarseSolveType='GMRES' "
                                  "has none")
    if singleDeviceSetup and not singlePrecision:
        raise NotImplementedError("singleDeviceSetup=True serves a ComplexF32 hierarchy (singlePrecision=True); Float64 and "
                                  "ComplexF64 hierarchies are refreshed on the device without it")
    if singleKcycle and not singlePrecision:
        raise NotImplementedError("singleKcycle=True serves a ComplexF32 hierarchy (singlePrecision=True); ComplexF64 hierarchies "
                                  "run the K-cycle and Jac-GMRES without it")
    if blockKcycle and np.dtype(VAL) != np.complex128:
        raise NotImplementedError("blockKcycle=True serves VAL=ComplexF64 (singlePrecision or not): blocks on a K-cycle / Jac-GMRES "
                                  "hierarchy are a feature of the complex path")
    if singlePrecision:
        VAL = np.complex64
    if np.dtype(IND) != np.int64:
        raise TypeError("only IND=Int64 is supported")
    pre = relaxPre if callable(relaxPre) else (lambda level, _k=int(relaxPre): _k)
    post = relaxPost if callable(relaxPost) else (lambda level, _k=int(relaxPost): _k)
    if cycleType not in ("V", "W", "F", "K"):
        raise ValueError("cycleType must be one of 'V','W','F','K'")
    return MGparam(levels=int(levels), numCores=int(numCores), maxOuterIter=int(maxIter),
                   relativeTol=float(relativeTol), relaxType=str(relaxType), relaxParam=relaxParam,
                   relaxPre=pre, relaxPost=post, cycleType=cycleType, coarseSolveType=str(coarseSolveType),
                   strongConnParam=float(strongConnParam), FilteringParam=float(FilteringParam),
                   transferOperatorType=str(transferOperatorType), singlePrecision=bool(singlePrecision),
                   blockCoarseGMRES=bool(blockCoarseGMRES), complexVanka=bool(complexVanka),
                   vankaBlocks=bool(vankaBlocks), vankaDeviceSetup=bool(vankaDeviceSetup),
                   coarseDeviceInverse=bool(coarseDeviceInverse), singleDeviceSetup=bool(singleDeviceSetup),
                   singleKcycle=bool(singleKcycle), blockKcycle=bool(blockKcycle), VAL=np.dtype(VAL).type, IND=np.int64)


def is_complex(param: MGparam) -> bool:
    """VAL = ComplexF64 or ComplexF32: the hierarchy is served by the _CF64 / _CF32 entry points."""
    return np.dtype(param.VAL) in (np.dtype(np.complex128), np.dtype(np.complex64))


def is_single(param: MGparam) -> bool:
    """VAL = ComplexF32 (getMGparam(np.complex128, ..., singlePrecision=True)): the _CF32 entry points."""
    return np.dtype(param.VAL) == np.complex64


def factor_val(param: MGparam):
    """The value type of the coarsest factorisation: Julia's lu of a ComplexF32 matrix factorises in double (MGsetup.jl:350)."""
    return np.dtype(np.complex128) if is_single(param) else np.dtype(param.VAL)


def factor_vals(param: MGparam):
    """The value types a ``parallelJuliaSolver`` preset as ``param.LU`` may hold: ``factor_val``, and on a ComplexF32 hierarchy
    ComplexF32 too - a single solver object (``getParallelJuliaSolver(np.complex64, ..., singleFactors=True)``), whose factors the
    coarsest solve applies to the cycle's own single vectors (mg_set_coarse_lu_CF32_INT64)."""
    return (factor_val(param), np.dtype(np.complex64)) if is_single(param) else (factor_val(param),)


def hierarchyExists(param: MGparam) -> bool:
    return len(param.As) > 0


def _solver_object(LU):
    """param.LU as a solver object preset before the setup (MGsetup.jl:323-331): 'dd', 'pjs' or None (a plain factorisation)."""
    from . import domain_decomposition as DD
    from . import parallel_julia_solver as PJS
    if isinstance(LU, DD.DomainDecompositionParam):
        return "dd"
    if isinstance(LU, PJS.parallelJuliaSolver):
        return "pjs"
    return None


def destroyCoarsestLU(param: MGparam) -> None:
    """MGdef.jl:191-206: a solver object is cleared and kept (l.200-201), a plain factorisation dropped."""
    kind = _solver_object(param.LU)
    if kind is None:
        param.LU = None
        return
    if param.device is not None:       # (the hierarchy gives a borrowed handle back before it is destroyed)
        _release_device(param)
    if kind == "dd":
        from .domain_decomposition import clear_ as clear_dd
        clear_dd(param.LU)
    else:
        from .parallel_julia_solver import clear_ as clear_pjs
        clear_pjs(param.LU)


def _release_device(param: MGparam) -> None:
    if param.device is not None:
        param.device.close()
        param.device = None


def clear_(param: MGparam) -> None:
    """``clear!(param)``: drop the hierarchy, the scratch memory and the device handle."""
    param.Ps, param.Rs, param.As = [], [], []
    param.relaxPrecs = []
    param.Meshes = []
    param.nrhs = 0
    destroyCoarsestLU(param)
    _release_device(param)


def copySolver(MG: MGparam) -> MGparam:
    """Copies the solver parameters without the setup and allocated memory (MGdef.jl:138-145); a solver-object ``LU`` is
    copied by its own ``copySolver`` (l.141-143), a plain factorisation is not."""
    single = is_single(MG)
    new = getMGparam(np.complex128 if single else MG.VAL, MG.IND, MG.levels, MG.numCores, MG.maxOuterIter, MG.relativeTol,
                     MG.relaxType, MG.relaxParam, MG.relaxPre, MG.relaxPost, MG.cycleType, MG.coarseSolveType,
                     MG.strongConnParam, MG.FilteringParam, MG.transferOperatorType, singlePrecision=single,
                     blockCoarseGMRES=bool(MG.blockCoarseGMRES), complexVanka=bool(MG.complexVanka),
                     vankaBlocks=bool(MG.vankaBlocks), vankaDeviceSetup=bool(MG.vankaDeviceSetup),
                     coarseDeviceInverse=bool(MG.coarseDeviceInverse), singleDeviceSetup=bool(MG.singleDeviceSetup),
                     singleKcycle=bool(MG.singleKcycle), blockKcycle=bool(MG.blockKcycle))
    kind = _solver_object(MG.LU)
    if kind == "dd":
        from .domain_decomposition import copySolver as copy_dd
        new.LU = copy_dd(MG.LU)
    elif kind == "pjs":
        from .parallel_julia_solver import copySolver as copy_pjs
        new.LU = copy_pjs(MG.LU)
    return new
