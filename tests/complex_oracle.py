"""TEST INFRASTRUCTURE ONLY.  numpy/scipy restatement of the multigrid cycle of JuliaInv/Multigrid.jl v0.8.0 for a complex
value type (VAL = ComplexF64), the checker of the _CF64 device path.  Imports no device code of the package.

The reference's solver is generic in VAL: MGparam{VAL,IND} (MGdef.jl:91-116), recursiveCycle / relax / solveCoarsest
(MGcycle.jl:1-181) and solveMG (SolveFuncs.jl:3-39) run on Array{VAL} unchanged.  Conventions here, as in the package:

  * ``param.As[l]`` is the APPLIED operator A = AT^H (scipy CSR, complex128): the reference applies its stored AT as
    ``mul!(target, adjoint(AT), x, alpha, beta)`` (SpMatMul.jl:9), i.e. y_i = sum_k conj(AT.nzval_k) x[AT.rowval_k] over
    CSC column i, which is the CSR product of A with A.data = conj(AT.nzval);
  * ``param.Ps`` / ``param.Rs`` are real (MGsetup.jl:80-81: Rs and Ps stay real(VAL));
  * ``param.relaxPrecs[l]`` is the complex d of ``x .+= d.*r`` (MGcycle.jl:129,134);
  * ``param.LU`` is a scipy splu of the coarsest A (``lu(sparse(AT'))``, MGsetup.jl:350);
  * norms are Julia's ``norm`` of a complex vector, sqrt(sum |z_i|^2) (SolveFuncs.jl:19,30).

Every function keeps the operation order of the reference lines it cites (the same order as oracle/mg_oracle.py, whose real
restatement this one must equal on real operators: tests/test_complex_host.py pins that).
"""
from __future__ import annotations

import numpy as np


def SpMatMul(alpha, A, x, beta, target):
    """target = beta*target + alpha*A*x (SpMatMul.jl:4-13), complex alpha / beta."""
    Ax = A @ x
    if beta == 0:
        target[...] = alpha * Ax
    else:
        target[...] = beta * target + alpha * Ax
    return target


def addVectors(alpha, x, target):
    """target += alpha*x (SpMatMul.jl:29-37)."""
    target += alpha * x


def relax(A, r, x, b, d, numit):
    """MGcycle.jl:122-136: numit-1 times {x .+= d.*r; r = -A x; r += b}, then x .+= d.*r (numit = 0 still updates once)."""
    for _ in range(1, numit):
        x += d * r                               # l.129
        SpMatMul(-1.0, A, x, 0.0, r)             # l.130
        addVectors(1.0, b, r)                    # l.131
    x += d * r                                   # l.134
    return x


def solveCoarsest(param, b, x):
    """Default branch: z = param.LU \\ b; x[:] = z (MGcycle.jl:177-178)."""
    x[...] = param.LU.solve(np.asarray(b, dtype=np.complex128))
    return x


class _Mem:
    """CYCLEmem per level (MGdef.jl:56-60), complex."""

    def __init__(self, param):
        self.r = [np.zeros(A.shape[0], dtype=np.complex128) for A in param.As]
        self.x = [np.zeros(A.shape[0], dtype=np.complex128) for A in param.As]
        self.b = [np.zeros(A.shape[0], dtype=np.complex128) for A in param.As]
        self.b[-1] = self.r[-1]                  # coarsest .b aliases .r (MGsetup.jl:217-218)


def recursiveCycle(param, b, x, level, mem=None, cycleType=None):
    """One cycle from `level` (1-based): MGcycle.jl:1-118 for the pointwise smoothers and the V / W / F cycles."""
    if mem is None:
        mem = _Mem(param)
    if cycleType is None:
        cycleType = param.cycleType
    As = param.As
    nlevels = len(As)
    if level == nlevels:                         # l.13-18
        r = mem.r[level - 1]
        r[...] = b
        return solveCoarsest(param, r, x)
    A = As[level - 1]
    r = mem.r[level - 1]
    r[...] = b                                   # l.26-28
    if np.linalg.norm(x) > 0.0:                  # l.29-31
        SpMatMul(-1.0, A, x, 1.0, r)
    D = param.relaxPrecs[level - 1]
    P = param.Ps[level - 1]
    R = param.Rs[level - 1]
    x = relax(A, r, x, b, D, param.relaxPre(level))          # l.54
    SpMatMul(-1.0, A, x, 0.0, r)                 # l.58
    addVectors(1.0, b, r)                        # l.60
    xc = mem.x[level]
    xc[...] = 0.0                                # l.63-64
    bc = mem.b[level]
    SpMatMul(1.0, R, r, 0.0, bc)                 # l.66
    if level == nlevels - 1:
        xc = solveCoarsest(param, bc, xc)        # l.67-69
    else:
        xc = recursiveCycle(param, bc, xc, level + 1, mem, cycleType)          # l.78
        if cycleType == "W":
            xc = recursiveCycle(param, bc, xc, level + 1, mem, "W")            # l.79-80
        elif cycleType == "F":
            xc = recursiveCycle(param, bc, xc, level + 1, mem, "V")            # l.81-84
    SpMatMul(1.0, P, xc, 1.0, x)                 # l.90
    r[...] = b                                   # l.92
    SpMatMul(-1.0, A, x, 1.0, r)                 # l.93
    x = relax(A, r, x, b, D, param.relaxPost(level))         # l.102
    return x


def solveMG(param, b, x, history=None):
    """SolveFuncs.jl:3-39; x updated in place.  Returns (x, iter); history (dict) receives resvec."""
    mem = _Mem(param)
    A = param.As[0]
    r = mem.r[0]
    r[...] = b                                   # l.14
    if np.linalg.norm(x) == 0:                   # l.15-21
        res = np.linalg.norm(b)
    else:
        SpMatMul(-1.0, A, x, 1.0, r)
        res = np.linalg.norm(r)
    res_init = res
    resvec = [res_init]
    it = 0
    for _ in range(param.maxOuterIter):          # l.23-37
        x = recursiveCycle(param, b, x, 1, mem)
        SpMatMul(-1.0, A, x, 0.0, r)
        addVectors(1.0, b, r)
        it += 1
        res = np.linalg.norm(r)
        resvec.append(res)
        if res / res_init < param.relativeTol:
            break
    if isinstance(history, dict):
        history["resvec"] = np.array(resvec)
    return x, it
