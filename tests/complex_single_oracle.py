"""TEST INFRASTRUCTURE ONLY.  numpy restatement of the multigrid cycle of JuliaInv/Multigrid.jl v0.8.0 for VAL = ComplexF32, the
checker of the _CF32 device path and of the mixed-precision preconditioner.  Imports no device code of the package.

What the reference does for VAL = ComplexF32 (getMGparam: singlePrecision, MGdef.jl:151): As are converted to VAL and Ps / Rs to
real(VAL) (MGsetup.jl:31-33, 79-82, 108-110), CYCLEmem holds Array{ComplexF32}, so recursiveCycle / relax run unchanged with every
product and sum in single precision; ``lu`` of the coarsest ComplexF32 matrix factorises in double (UMFPACK has no single form,
MGsetup.jl:350) and ``param.LU \\ b`` is converted back when it is stored into x (MGcycle.jl:177-178).  The mixed closure of
getMultigridPreconditioner (SolveFuncs.jl:52-58) is ``bl .= b; recursiveCycle(param, bl, z, 1); z2 .= z``.

Here every operand and every intermediate is complex64 / float32 (asserted where a silent promotion could creep in); the coarsest
solve runs through ``param.LU`` (a complex128 splu) and is converted back.  The operation order is that of tests/complex_oracle.py,
whose SpMatMul / addVectors / relax are dtype-generic and are used as they are.  Norms are accumulated in double, as the device does.

``rounded(param)`` is the same hierarchy widened back to complex128 / float64: tests/complex_oracle.py on it is the double-precision
cycle on single-rounded data, the comparand of the single cycle.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import complex_krylov_oracle as ck
import complex_oracle as corc
from complex_cases import complex_rhs, helmholtz

C64 = np.complex64
U32 = 2.0 ** -24


def _single(*arrs):
    for a in arrs:
        assert a.dtype == C64, a.dtype


def solveCoarsest(param, b, x):
    """z = param.LU \\ b in double; x[:] = z converts back (MGcycle.jl:177-178)."""
    x[...] = param.LU.solve(np.asarray(b, dtype=np.complex128)).astype(C64)
    return x


class _Mem:
    """CYCLEmem per level (MGdef.jl:56-60), ComplexF32."""

    def __init__(self, param):
        self.r = [np.zeros(A.shape[0], dtype=C64) for A in param.As]
        self.x = [np.zeros(A.shape[0], dtype=C64) for A in param.As]
        self.b = [np.zeros(A.shape[0], dtype=C64) for A in param.As]
        self.b[-1] = self.r[-1]


def recursiveCycle(param, b, x, level, mem=None, cycleType=None):
    """tests/complex_oracle.py's recursiveCycle line by line, on complex64 arrays."""
    if mem is None:
        mem = _Mem(param)
    if cycleType is None:
        cycleType = param.cycleType
    As = param.As
    nlevels = len(As)
    _single(b, x)
    if level == nlevels:
        r = mem.r[level - 1]
        r[...] = b
        return solveCoarsest(param, r, x)
    A = As[level - 1]
    D = param.relaxPrecs[level - 1]
    P = param.Ps[level - 1]
    R = param.Rs[level - 1]
    assert A.dtype == C64 and D.dtype == C64 and P.dtype == np.float32 and R.dtype == np.float32
    r = mem.r[level - 1]
    r[...] = b
    if np.linalg.norm(x) > 0.0:
        corc.SpMatMul(-1.0, A, x, 1.0, r)
    x = corc.relax(A, r, x, b, D, param.relaxPre(level))
    corc.SpMatMul(-1.0, A, x, 0.0, r)
    corc.addVectors(1.0, b, r)
    xc = mem.x[level]
    xc[...] = 0.0
    bc = mem.b[level]
    corc.SpMatMul(1.0, R, r, 0.0, bc)
    if level == nlevels - 1:
        xc = solveCoarsest(param, bc, xc)
    else:
        xc = recursiveCycle(param, bc, xc, level + 1, mem, cycleType)
        if cycleType == "W":
            xc = recursiveCycle(param, bc, xc, level + 1, mem, "W")
        elif cycleType == "F":
            xc = recursiveCycle(param, bc, xc, level + 1, mem, "V")
    corc.SpMatMul(1.0, P, xc, 1.0, x)
    r[...] = b
    corc.SpMatMul(-1.0, A, x, 1.0, r)
    x = corc.relax(A, r, x, b, D, param.relaxPost(level))
    _single(x, r, bc, xc)
    return x


def norm(z):
    """sqrt(sum |z_i|^2) of a complex64 vector, squares and sum in double."""
    z = np.asarray(z)
    return float(np.sqrt(np.sum(z.real.astype(np.float64) ** 2 + z.imag.astype(np.float64) ** 2)))


def solveMG(param, b, x, history=None):
    """SolveFuncs.jl:3-39 on complex64 vectors; x updated in place.  Returns (x, iter)."""
    mem = _Mem(param)
    A = param.As[0]
    _single(b, x)
    r = mem.r[0]
    r[...] = b
    if norm(x) == 0:
        res = norm(b)
    else:
        corc.SpMatMul(-1.0, A, x, 1.0, r)
        res = norm(r)
    res_init = res
    resvec = [res_init]
    it = 0
    for _ in range(param.maxOuterIter):
        x = recursiveCycle(param, b, x, 1, mem)
        corc.SpMatMul(-1.0, A, x, 0.0, r)
        corc.addVectors(1.0, b, r)
        it += 1
        res = norm(r)
        resvec.append(res)
        if res / res_init < param.relativeTol:
            break
    if isinstance(history, dict):
        history["resvec"] = np.array(resvec)
    return x, it


def rounded(param):
    """The hierarchy of a single param widened back to complex128 / float64 (the values stay the single-rounded ones), in the
    shape tests/complex_oracle.py reads."""
    return SimpleNamespace(As=[A.astype(np.complex128) for A in param.As], Ps=[P.astype(np.float64) for P in param.Ps],
                           Rs=[R.astype(np.float64) for R in param.Rs],
                           relaxPrecs=[d.astype(np.complex128) for d in param.relaxPrecs], LU=param.LU,
                           relaxPre=param.relaxPre, relaxPost=param.relaxPost, cycleType=param.cycleType,
                           maxOuterIter=param.maxOuterIter, relativeTol=param.relativeTol)


def preconditioner(param):
    """The mixed closure (SolveFuncs.jl:52-58): bl .= b; z .= 0; recursiveCycle(param, bl, z, 1); z2 .= z."""
    mem = _Mem(param)

    def M(v):
        bl = np.asarray(v, dtype=np.complex128).astype(C64)
        z = np.zeros(bl.shape[0], dtype=C64)
        return recursiveCycle(param, bl, z, 1, mem).astype(np.complex128)

    return M


def rel2(a, ref):
    """relative 2-norm distance, in double"""
    a = np.asarray(a, dtype=np.complex128)
    ref = np.asarray(ref, dtype=np.complex128)
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


# ---- the shared cases of tests/complex_krylov_oracle.py with a ComplexF32 hierarchy ---------------------------------------------
_cache = {}


def case(mg, name):
    """(param, A_sys, b) as complex_krylov_oracle.case, the hierarchy built with singlePrecision=True.  Built once per process and
    shared - nothing in it may be modified."""
    if name not in _cache:
        cells, levels, damp = ck.CASES[name]
        Ah, mesh = helmholtz(mg, [cells] * 3, 0.5, 0.5)
        p = mg.getMGparam(np.complex128, np.int64, levels, 8, ck.MAXIT_BICGSTAB, ck.TOL, "SPAI", 1.0, 2, 1, "V", "NoMUMPS", 0.5, 0.0,
                          singlePrecision=True)
        mg.MGsetup(Ah, mesh, p)
        As, _ = helmholtz(mg, [cells] * 3, 0.5, damp)
        _cache[name] = (p, As, complex_rhs(Ah.shape[0], 21))
    return _cache[name]


_runs = {}


def reference(mg, name, method, inner=None, x0=None, maxIter=None, key=None, rhs=None):
    """The complex128 oracle drivers with the single restatement as M on a case, computed once and shared:
    (x, flag, count, resvec)."""
    k = (name, method, inner, key)
    if k not in _runs:
        p, As, b = case(mg, name)
        if rhs is not None:
            b = rhs
        Afun = lambda v: As @ v
        M = preconditioner(p)
        if method == "bicgstab":
            _runs[k] = ck.bicgstb(Afun, b, ck.TOL, ck.MAXIT_BICGSTAB if maxIter is None else maxIter, M, x0)
        else:
            _runs[k] = ck.fgmres(Afun, b, inner, ck.TOL, ck.MAXIT_FGMRES if maxIter is None else maxIter, M, x0)
    return _runs[k]
