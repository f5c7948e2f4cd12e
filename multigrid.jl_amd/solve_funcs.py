"""Host-side mirror of the reference's cycle API: every call goes to the HIP library.

Mirrors reference src/Multigrid/SolveFuncs.jl:3-39 (``solveMG``), MGcycle.jl:1-118 (``recursiveCycle``),
SpMatMul.jl:4-26 (``SpMatMul``) and SolveFuncs.jl:43-63 (``getMultigridPreconditioner``).
Same names, argument meaning and in-place contract; the arithmetic runs on the MI355X only.
"""
from __future__ import annotations

import numpy as np

from .device import DeviceHierarchy, MG_OP_A, MG_OP_P, MG_OP_R
from .mgdef import MGparam, hierarchyExists, is_complex, is_single
from .mgsetup import adjustMemoryForNumRHS


def _real_only(param: MGparam, what: str):
    if is_complex(param):
        raise NotImplementedError(f"{what}: this driver serves VAL=Float64; a ComplexF64 hierarchy takes solveBiCGSTAB_MG_CFP64 / "
                                  "solveGMRES_MG_CFP64 (or precondition a Krylov method of your own with getMultigridPreconditioner)")


def _ncols(b):
    return 1 if b.ndim == 1 else int(b.shape[1])


def _complex_block(param: MGparam, b) -> bool:
    """A complex hierarchy given more than one column: the device's block entry points take the column count with each call and
    the handle's own nrhs stays 1 (``adjustMemoryForNumRHS(param, 1)``)."""
    return is_complex(param) and _ncols(b) > 1


def _coarse_gmres_guard(param: MGparam, b) -> None:
    """A complex hierarchy with coarseSolveType='GMRES' given a block: the reference calls blockFGMRES in its coarsest solve
    (MGcycle.jl:166-167).  That form runs only where the param asked for it (``getMGparam(..., blockCoarseGMRES=True)``); without
    it the block is refused before the device is touched, as the device layer refuses it."""
    from .mgdef import _solver_object
    if param.blockCoarseGMRES:
        return
    if _complex_block(param, b) and param.coarseSolveType == "GMRES" and _solver_object(param.LU) is None:
        raise NotImplementedError("blocks of right-hand sides are not served on a complex hierarchy with coarseSolveType='GMRES' "
                                  "(solve the columns one after the other)")


def _vanka_block_guard(param: MGparam, b) -> None:
    """A complex Vanka hierarchy given more than one column: refused before the device is touched (a real one is refused by
    ``_vanka_guard`` through the handle's nrhs) unless the param asked for the block form of the smoother
    (``getMGparam(..., complexVanka=True, vankaBlocks=True)``)."""
    from .mgsetup import _is_vanka
    if not (_complex_block(param, b) and _is_vanka(param)):
        return
    if not getattr(param, "vankaBlocks", False):
        raise NotImplementedError("blocks of right-hand sides are not served on a complex Vanka hierarchy (solve the columns one "
                                  "after the other)")
    # vankaBlocks=True: the block form of the smoother serves the block; what it does not serve is refused here, before the device
    from .device import BLOCK_KMAX
    from .mgdef import _solver_object
    if _ncols(b) > BLOCK_KMAX:
        raise NotImplementedError(f"complex Vanka hierarchies serve blocks of at most {BLOCK_KMAX} right-hand sides ({_ncols(b)} given)")
    if np.asarray(b).dtype.kind != "c":
        raise NotImplementedError("a real block on a complex Vanka hierarchy is not served (blocks of a complex hierarchy are complex128)")
    if param.cycleType == "K":
        raise NotImplementedError("blocks of right-hand sides are not served on a K-cycle complex Vanka hierarchy")
    if _solver_object(param.LU) == "dd":
        raise NotImplementedError("complex Vanka hierarchies: a Schwarz coarsest solve is out of scope")


def _width(param: MGparam, b) -> int:
    """The nrhs the handle is sized for: the block's columns, or 1 for a complex hierarchy (see ``_complex_block``)."""
    return 1 if is_complex(param) else _ncols(b)


def to_device(param: MGparam, device_id: int = 0) -> DeviceHierarchy:
    """Upload the hierarchy (lifecycle hook at the end of MGsetup/SA_AMGsetup, MGsetup.jl:135-137)."""
    if not hierarchyExists(param):
        raise RuntimeError("The Hierarchy is empty - run a setup first.")
    from .device import _vanka_guard
    _vanka_guard(param, max(1, param.nrhs))       # what a Vanka hierarchy does not serve: refused before the device is touched
    if param.device is None:
        param.device = DeviceHierarchy(param, device_id=device_id, nrhs=max(1, param.nrhs))
    else:
        # the reference reads cycleType / relaxType / relaxPre / relaxPost from param on every cycle
        # (MGcycle.jl:44-45,72-85): follow changes made after the upload
        param.device.sync_schedule(param)
    return param.device


def solveMG(param: MGparam, b: np.ndarray, x: np.ndarray, verbose: bool = False):
    """``(x, param, iter) = solveMG(param,b,x,verbose)``: x is updated IN PLACE (testGMG.jl:54-55)."""
    _vanka_block_guard(param, b)
    _coarse_gmres_guard(param, b)
    adjustMemoryForNumRHS(param, _width(param, b))
    dev = to_device(param)
    if _complex_block(param, b):                  # the residual norms are Frobenius norms of the block (SolveFuncs.jl:14-36)
        _, iters, resvec = dev.block_solve(b, x, param.relativeTol, param.maxOuterIter)
    else:
        _, iters, resvec = dev.solve(b, x, param.relativeTol, param.maxOuterIter)
    param.resvec = resvec
    if verbose:
        for c in range(1, iters + 1):
            print(f"Cycle {c} done with relres: {resvec[c] / resvec[0]}. Convergence factor: {resvec[c] / resvec[c - 1]}")
    return x, param, iters


def recursiveCycle(param: MGparam, b: np.ndarray, x: np.ndarray, level: int = 1):
    """One cycle from the finest level.  Only ``level == 1`` is an entry point of the device library."""
    if level != 1:
        raise ValueError("the device library owns the recursion: only level=1 can be entered from the host")
    _vanka_block_guard(param, b)
    _coarse_gmres_guard(param, b)
    adjustMemoryForNumRHS(param, _width(param, b))
    if _complex_block(param, b):
        to_device(param).block_cycle(b, x, -1)
    else:
        to_device(param).cycle(b, x, -1)
    return x


def getMultigridPreconditioner(param: MGparam, B: np.ndarray, verbose: bool = False):
    """``M(b) = (z .= 0; recursiveCycle(param,b,z,1); z)`` (SolveFuncs.jl:59): x = 0 on entry."""
    if not hierarchyExists(param):
        print("You have to do a setup first.")
    _vanka_block_guard(param, B)
    _coarse_gmres_guard(param, B)
    adjustMemoryForNumRHS(param, _width(param, B))
    dev = to_device(param)
    if _complex_block(param, B):
        return _complex_block_preconditioner(param, dev, B)
    if B.dtype == np.float32:            # mixed precision (SolveFuncs.jl:52-58): bl .= b; cycle in Float64; z2 .= z
        z2 = np.zeros_like(B, order="F")

        def MMG32(b):
            dev.cycle_mixed_f32(np.asfortranarray(b, dtype=np.float32), z2)
            return z2

        return MMG32
    if is_single(param):
        # ComplexF32 hierarchy.  complex128 B: the mixed branch VAL != eltype(B) (SolveFuncs.jl:52-58) - bl .= b; the single cycle
        # from zero; z2 .= z - so the closure preconditions a ComplexF64 Krylov method.  complex64 B: the plain closure below.
        if B.dtype == np.complex128:
            bl = np.zeros(B.shape, dtype=np.complex64, order="F")
            zl = np.zeros_like(bl)
            z2 = np.zeros_like(B, order="F")

            def MMGmixed(b):
                bl[...] = b
                zl[...] = 0.0
                dev.cycle(bl, zl, 1)
                z2[...] = zl
                return z2

            return MMGmixed
        if B.dtype != np.complex64:
            raise TypeError("getMultigridPreconditioner of a ComplexF32 hierarchy takes a complex128 (mixed) or complex64 B")
    z = np.zeros_like(B, order="F")

    def MMG(b):
        z[...] = 0.0
        dev.cycle(np.asfortranarray(b), z, 1)
        return z

    return MMG


def _complex_block_preconditioner(param: MGparam, dev, B: np.ndarray):
    """getMultigridPreconditioner for a complex hierarchy and a block of more than one column: one cycle on the whole block from
    zero.  A ComplexF32 hierarchy takes a complex128 block - the mixed closure (SolveFuncs.jl:52-58) on the whole block, run on
    device blocks (narrowed, cycled and widened in HBM)."""
    if B.dtype != np.complex128:
        raise TypeError("getMultigridPreconditioner: blocks of a complex hierarchy are complex128 (ComplexF32 hierarchies: the mixed closure)")
    z = np.zeros(B.shape, dtype=np.complex128, order="F")
    if not is_single(param):

        def MMGblock(b):
            z[...] = 0.0
            dev.block_cycle(np.asfortranarray(b, dtype=np.complex128), z, 1)
            return z

        return MMGblock
    import torch

    def MMGblockMixed(b):
        bd = torch.from_numpy(np.ascontiguousarray(b, dtype=np.complex128)).to(f"cuda:{torch.cuda.current_device()}")   # row-major [n][k]
        zd = torch.zeros_like(bd)
        dev.block_cycle_dev(bd, zd, 1)
        torch.cuda.synchronize()
        z[...] = zd.cpu().numpy()
        return z

    return MMGblockMixed


def solveCG_MG(A, param: MGparam, b: np.ndarray, x0: np.ndarray, verbose: bool = False):
    """``(x, param, iter) = solveCG_MG(AT,param,b,x0,verbose)`` (SolveFuncs.jl:104-116): KrylovMethods.cg with
    the multigrid cycle as preconditioner, vectors resident on the device across iterations.  ``A`` is accepted
    for signature parity; the operator applied is ``param.As[1]`` on the device (the reference passes the same
    matrix twice).  x0 is updated in place.  ``size(b,2) > 1`` takes the blockCG branch (l.113), also on the device."""
    _real_only(param, "solveCG_MG")
    adjustMemoryForNumRHS(param, _ncols(b))
    dev = to_device(param)
    x, flag, it, resvec = dev.pcg(b, x0, param.relativeTol, param.maxOuterIter)
    param.resvec = resvec
    param.flag = flag
    if verbose:
        for k, r in enumerate(resvec):
            print(f"{k + 1:3d}\t{r:1.2e}")
    return x, param, it


def solveBiCGSTAB_MG(A, param: MGparam, b: np.ndarray, x0: np.ndarray, verbose: bool = False):
    """``(x, param, iter, nprec) = solveBiCGSTAB_MG(AT,param,b,x0,verbose)`` (SolveFuncs.jl:87-101): KrylovMethods.bicgstb
    with M1 = the multigrid cycle, M2 = identity, on the device; blocks take the blockBiCGSTB branch (l.95)."""
    _real_only(param, "solveBiCGSTAB_MG")
    adjustMemoryForNumRHS(param, _ncols(b))
    dev = to_device(param)
    x, flag, it, resvec = dev.bicgstab(b, x0, param.relativeTol, param.maxOuterIter)
    param.resvec = resvec
    param.flag = flag
    nprec = 2 * it * _ncols(b) + (flag == -3) * _ncols(b)        # SolveFuncs.jl:99 as written
    return x, param, it, nprec


def solveGMRES_MG(A, param: MGparam, b: np.ndarray, x0: np.ndarray, flexible: bool, inner: int, verbose: bool = False):
    """``(x, param, iter, resvec) = solveGMRES_MG(AT,param,b,x0,flexible,inner,verbose)`` (SolveFuncs.jl:119-133):
    KrylovMethods.fgmres with the multigrid cycle as preconditioner on the device (always the flexible variant: the
    cycle is a fixed linear operator, so flexible and standard GMRES generate the same iterates); blocks take the
    blockFGMRES branch (l.130)."""
    _real_only(param, "solveGMRES_MG")
    adjustMemoryForNumRHS(param, _ncols(b))
    dev = to_device(param)
    x, flag, it, resvec = dev.fgmres(b, x0, inner, param.relativeTol, param.maxOuterIter)
    param.resvec = resvec
    param.flag = flag
    return x, param, it, resvec


def _complex_krylov_device(A, param: MGparam, b, x0, what: str):
    """What the two _CFP64 functions share: the checks, the upload of the hierarchy and - when it is not the object uploaded
    last - of the system operator A (None or ``param.As[0]`` itself: the hierarchy's own fine level)."""
    if not is_complex(param):
        raise TypeError(f"{what} serves VAL=ComplexF64 hierarchies; a Float64 hierarchy goes to {what[:-len('_CFP64')]}")
    if _ncols(b) != 1 or _ncols(x0) != 1:
        raise NotImplementedError(f"{what}: one right-hand side (blocks of right-hand sides are not served for complex values)")
    adjustMemoryForNumRHS(param, 1)
    dev = to_device(param)
    if A is not None and param.As and A is param.As[0]:
        A = None
    if A is not dev.krylov_operator:          # recorded by set_krylov_operator itself: a direct call to it is seen here
        dev.update_krylov_operator(A)         # (the pattern uploaded last: new values only)
    return dev, b.reshape(-1) if b.ndim == 2 else b, x0.reshape(-1) if x0.ndim == 2 else x0


def solveBiCGSTAB_MG_CFP64(A, param: MGparam, b: np.ndarray, x0: np.ndarray, verbose: bool = False):
    """``(x, param, iter, nprec) = solveBiCGSTAB_MG(Afun,param,b,x0,verbose)`` (SolveFuncs.jl:87-101) for VAL = ComplexF64 on the
    device: KrylovMethods.bicgstb on the system operator ``A`` - the APPLIED operator, the convention of ``param.As``: a scipy
    sparse matrix, complex or real; None or ``param.As[0]`` for the hierarchy's own fine level - with one cycle of ``param``'s
    hierarchy (typically built on a damped copy of A) as M1.  x0 is updated in place; one right-hand side."""
    dev, bv, xv = _complex_krylov_device(A, param, b, x0, "solveBiCGSTAB_MG_CFP64")
    _, flag, it, resvec = dev.bicgstab(bv, xv, param.relativeTol, param.maxOuterIter)
    param.resvec = resvec
    param.flag = flag
    if verbose:
        for k, r in enumerate(resvec):
            print(f"{k:3d}\t{r:1.2e}")
    nprec = 2 * it + (flag == -3)                                   # SolveFuncs.jl:99 as written
    return x0, param, it, nprec


def solveGMRES_MG_CFP64(A, param: MGparam, b: np.ndarray, x0: np.ndarray, flexible: bool, inner: int, verbose: bool = False):
    """``(x, param, iter, resvec) = solveGMRES_MG(Afun,param,b,x0,flexible,inner,verbose)`` (SolveFuncs.jl:119-133) for
    VAL = ComplexF64 on the device: KrylovMethods.fgmres(inner) on the system operator ``A`` (as for solveBiCGSTAB_MG_CFP64)
    with one cycle as preconditioner; always the flexible variant, as solveGMRES_MG.  x0 is updated in place."""
    dev, bv, xv = _complex_krylov_device(A, param, b, x0, "solveGMRES_MG_CFP64")
    _, flag, it, resvec = dev.fgmres(bv, xv, inner, param.relativeTol, param.maxOuterIter)
    param.resvec = resvec
    param.flag = flag
    if verbose:
        for k, r in enumerate(resvec):
            print(f"{k + 1:3d}\t{r:1.2e}")
    return x0, param, it, resvec


def solveBlockBiCGSTAB_MG_CFP64(A, param: MGparam, B: np.ndarray, X0: np.ndarray, verbose: bool = False):
    """``(X, param, iter, nprec) = solveBiCGSTAB_MG(Afun,param,B,X0,verbose)`` with ``size(B,2) > 1`` (SolveFuncs.jl:94-99) for
    VAL = ComplexF64 / ComplexF32 on the device: KrylovMethods.blockBiCGSTB on the whole n x k block (k <= 16; one column is legal),
    system operator ``A`` as for solveBiCGSTAB_MG_CFP64, one block cycle as M1.  X0 is updated in place;
    ``nprec = 2*iter*k + (flag == -3)*k``."""
    if not is_complex(param):
        raise TypeError("solveBlockBiCGSTAB_MG_CFP64 serves VAL=ComplexF64 hierarchies; a Float64 hierarchy goes to solveBiCGSTAB_MG")
    if _ncols(B) != _ncols(X0):
        raise ValueError("B and X0 must hold the same number of columns")
    _vanka_block_guard(param, B)
    _coarse_gmres_guard(param, B)
    adjustMemoryForNumRHS(param, 1)               # the block entry points take the column count with each call
    dev = to_device(param)
    if A is not None and param.As and A is param.As[0]:
        A = None
    if A is not dev.krylov_operator:
        dev.update_krylov_operator(A)
    k = _ncols(B)
    _, flag, it, resvec = dev.block_bicgstab(B, X0, param.relativeTol, param.maxOuterIter)
    param.resvec = resvec
    param.flag = flag
    if verbose:
        for j, r in enumerate(resvec):
            print(f"{j:3d}\t{r:1.2e}")
    nprec = 2 * it * k + (flag == -3) * k                           # SolveFuncs.jl:97 as written
    return X0, param, it, nprec


def solveBlockGMRES_MG_CFP64(A, param: MGparam, B: np.ndarray, X0: np.ndarray, flexible: bool, inner: int, verbose: bool = False):
    """``(X, param, iter, resvec) = solveGMRES_MG(Afun,param,B,X0,flexible,inner,verbose)`` with ``size(B,2) > 1`` (SolveFuncs.jl:130)
    for VAL = ComplexF64 / ComplexF32 on the device: KrylovMethods.blockFGMRES(inner) on the whole n x k block (k <= 16; one column is
    legal), system operator ``A`` as for solveBiCGSTAB_MG_CFP64, one block cycle as preconditioner; always the flexible variant.  X0 is
    updated in place; ``iter`` counts the inner steps and ``resvec`` holds ``||xi - H Y||_F / ||B||_F`` of each."""
    if not is_complex(param):
        raise TypeError("solveBlockGMRES_MG_CFP64 serves VAL=ComplexF64 hierarchies; a Float64 hierarchy goes to solveGMRES_MG")
    if _ncols(B) != _ncols(X0):
        raise ValueError("B and X0 must hold the same number of columns")
    _vanka_block_guard(param, B)
    _coarse_gmres_guard(param, B)
    adjustMemoryForNumRHS(param, 1)               # the block entry points take the column count with each call
    dev = to_device(param)
    if A is not None and param.As and A is param.As[0]:
        A = None
    if A is not dev.krylov_operator:
        dev.update_krylov_operator(A)
    _, flag, it, resvec = dev.block_fgmres(B, X0, inner, param.relativeTol, param.maxOuterIter)
    param.resvec = resvec
    param.flag = flag
    if verbose:
        for j, r in enumerate(resvec):
            print(f"{j + 1:3d}\t{r:1.2e}")
    return X0, param, it, resvec


_WHICH = {"A": MG_OP_A, "P": MG_OP_P, "R": MG_OP_R}


def SpMatMul(param: MGparam, level: int, which: str, x: np.ndarray, target: np.ndarray,
             alpha: float = 1.0, beta: float = 0.0):
    """``target = beta*target + alpha*Op*x`` (SpMatMul.jl:4-13) with Op = As/Ps/Rs[level] resident on device."""
    _vanka_block_guard(param, x)
    _coarse_gmres_guard(param, x)
    adjustMemoryForNumRHS(param, _width(param, x))
    if _complex_block(param, x):
        to_device(param).block_spmv(level, _WHICH[which], alpha, x, beta, target)
    else:
        to_device(param).spmv(level, _WHICH[which], alpha, x, beta, target)
    return target
