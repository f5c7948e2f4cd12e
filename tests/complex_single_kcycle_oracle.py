"""TEST INFRASTRUCTURE ONLY.  tests/complex_single_oracle.py's recursiveCycle (VAL = ComplexF32) with the Jac-GMRES and K branches
of tests/complex_kcycle_oracle.py, under the DEVICE'S ARITHMETIC CONTRACT for a ``singleKcycle`` hierarchy.  Imports no device code
of the package.

The contract (include/mgvcycle.h, mg_set_schedule_CF32):
  * Z and AZ are complex64; w = A z and the next direction d.*w are formed in single, through the dtype-generic SpMatMul of
    tests/complex_oracle.py and numpy's complex64 product;
  * H, xi and ||r0|| are formed in DOUBLE from those complex64 values (each product of two singles is exact in double);
  * julia_pinv, t and the residual estimate rn are double - complex_kcycle_oracle's host algebra, unchanged;
  * x += Z t is formed per element in double and rounded to single ONCE.
This is a deliberate deviation from the reference, which forms H in ComplexF32 - there rn cancels down to about
sqrt(2^-24) ||r0|| and the break at rn < 1e-5 is noise.

``FGMRES_relaxation`` below is complex_kcycle_oracle.FGMRES_relaxation itself, handed an operator and a preconditioner that work in
single and return their complex64 results widened: its double arrays Z / AZ then hold complex64 values exactly, and its dots, its
least squares and its update are the contract's.  ``trace`` records what complex_kcycle_oracle records."""
from __future__ import annotations

import numpy as np

import complex_kcycle_oracle as korc
import complex_oracle as corc
import complex_single_oracle as cs

C64 = np.complex64
C128 = np.complex128
GMRES_TOL = korc.GMRES_TOL


def _narrow(v):
    """complex128 -> complex64 of a vector that holds single values: exact (asserted)."""
    s = np.asarray(v).astype(C64)
    assert np.array_equal(s.astype(C128), v), "a direction of the relaxation is not a complex64 vector"
    return s


def FGMRES_relaxation(Afun, r0, x0, inner, prec, TOL, record=None, bases=None):
    """x0 += Z t for complex64 r0 and x0 (x0 updated in place).  Afun and prec map complex64 to complex64.  Returns (x0, rnorms);
    ``bases`` (a dict) receives H, xi (double), Z and AZ (complex64) of the directions computed."""
    cs._single(r0, x0)
    keepZ, keepAZ = [], []

    def A64(z):
        w = Afun(_narrow(z))
        cs._single(w)
        keepAZ.append(w.copy())
        return w.astype(C128)

    def P64(v):
        z = prec(_narrow(v))
        cs._single(z)
        keepZ.append(z.copy())
        return z.astype(C128)

    xw, rnorms = korc.FGMRES_relaxation(A64, r0.astype(C128), x0.astype(C128), inner, P64, TOL, record)
    x0[...] = xw.astype(C64)                     # the element's sum in double, rounded once
    if bases is not None and inner > 0:
        AZ = np.stack(keepAZ, axis=1)
        W = AZ.astype(C128)
        bases.update(Z=np.stack(keepZ, axis=1), AZ=AZ, H=W.conj().T @ W, xi=W.conj().T @ r0.astype(C128))
    return x0, rnorms


def _spmv(A):
    """w = A z in single through SpMatMul (complex64 in, complex64 out)."""
    def f(z):
        w = np.zeros(A.shape[0], dtype=C64)
        corc.SpMatMul(1.0, A, z, 0.0, w)
        return w
    return f


def recursiveCycle(param, b, x, level, mem=None, cycleType=None, trace=None):
    """complex_single_oracle.recursiveCycle with the Jac-GMRES (MGcycle.jl:35-50,96-98) and K (l.72-76) branches."""
    if mem is None:
        mem = cs._Mem(param)
    if cycleType is None:
        cycleType = param.cycleType
    As = param.As
    nlevels = len(As)
    cs._single(b, x)
    if level == nlevels:
        r = mem.r[level - 1]
        r[...] = b
        return cs.solveCoarsest(param, r, x)
    A = As[level - 1]
    D = param.relaxPrecs[level - 1]
    P = param.Ps[level - 1]
    R = param.Rs[level - 1]
    assert A.dtype == C64 and D.dtype == C64 and P.dtype == np.float32 and R.dtype == np.float32
    r = mem.r[level - 1]
    r[...] = b
    if np.linalg.norm(x) > 0.0:
        corc.SpMatMul(-1.0, A, x, 1.0, r)
    npre, npost = param.relaxPre(level), param.relaxPost(level)
    gmres_relax = param.relaxType == "Jac-GMRES"
    MM = lambda v: D * v
    Afun = _spmv(A)

    def note(kind, inner, rec):
        if trace is not None and rec:
            trace.append((kind, level, inner, rec[0][0], rec[0][1]))

    if gmres_relax:
        rec = []
        x = FGMRES_relaxation(Afun, r, x, npre, MM, GMRES_TOL, rec)[0]
        note("pre", npre, rec)
    else:
        x = corc.relax(A, r, x, b, D, npre)
    corc.SpMatMul(-1.0, A, x, 0.0, r)
    corc.addVectors(1.0, b, r)
    xc = mem.x[level]
    xc[...] = 0.0
    bc = mem.b[level]
    corc.SpMatMul(1.0, R, r, 0.0, bc)
    if level == nlevels - 1:
        xc = cs.solveCoarsest(param, bc, xc)
    elif cycleType == "K":
        def MMG(v):
            return recursiveCycle(param, v, np.zeros_like(v), level + 1, mem, "K", trace).copy()

        rec = []
        xc = FGMRES_relaxation(_spmv(As[level]), bc.copy(), xc, 2, MMG, GMRES_TOL, rec)[0]
        note("K", 2, rec)
    else:
        xc = recursiveCycle(param, bc, xc, level + 1, mem, cycleType, trace)
        if cycleType == "W":
            xc = recursiveCycle(param, bc, xc, level + 1, mem, "W", trace)
        elif cycleType == "F":
            xc = recursiveCycle(param, bc, xc, level + 1, mem, "V", trace)
    corc.SpMatMul(1.0, P, xc, 1.0, x)
    r[...] = b
    corc.SpMatMul(-1.0, A, x, 1.0, r)
    if gmres_relax:
        rec = []
        x = FGMRES_relaxation(Afun, r, x, npost, MM, GMRES_TOL, rec)[0]
        note("post", npost, rec)
    else:
        x = corc.relax(A, r, x, b, D, npost)
    cs._single(x, r, bc, xc)
    return x


def solveMG(param, b, x, history=None, trace=None):
    """complex_single_oracle.solveMG with the cycle above.  Returns (x, iter)."""
    mem = cs._Mem(param)
    A = param.As[0]
    cs._single(b, x)
    r = mem.r[0]
    r[...] = b
    if cs.norm(x) == 0:
        res = cs.norm(b)
    else:
        corc.SpMatMul(-1.0, A, x, 1.0, r)
        res = cs.norm(r)
    res_init = res
    resvec = [res_init]
    it = 0
    for _ in range(param.maxOuterIter):
        x = recursiveCycle(param, b, x, 1, mem, None, trace)
        corc.SpMatMul(-1.0, A, x, 0.0, r)
        corc.addVectors(1.0, b, r)
        it += 1
        res = cs.norm(r)
        resvec.append(res)
        if res / res_init < param.relativeTol:
            break
    if isinstance(history, dict):
        history["resvec"] = np.array(resvec)
    return x, it


def rounded(param):
    """complex_single_oracle.rounded with the relaxType complex_kcycle_oracle reads."""
    q = cs.rounded(param)
    q.relaxType = param.relaxType
    return q


def preconditioner(param, trace=None):
    """The mixed closure (SolveFuncs.jl:52-58) around the cycle above."""
    mem = cs._Mem(param)

    def M(v):
        bl = np.asarray(v, dtype=C128).astype(C64)
        z = np.zeros(bl.shape[0], dtype=C64)
        return recursiveCycle(param, bl, z, 1, mem, None, trace).astype(C128)

    return M
