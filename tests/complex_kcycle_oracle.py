"""TEST INFRASTRUCTURE ONLY.  The complex oracle (tests/complex_oracle.py) with the two branches it leaves out: Jac-GMRES
smoothing (MGcycle.jl:35-50,96-98) and the K-cycle (MGcycle.jl:72-76), both through FGMRES_relaxation (FGMRES.jl:48-126) for
VAL = ComplexF64.  Imports no device code of the package.

Every function keeps the operation order of the reference lines it cites.  Julia's ``dot`` and ``gemv!('C', ...)`` conjugate
their first argument; ``H[j,:] = t'`` writes the conjugate.  ``pinv`` is Julia's: singular values below eps * size * sigma_max
are dropped.  ``trace`` (a list) receives one record per relaxation: (kind, level, inner, used, [rn ...]) with kind "pre",
"post" or "K" - every residual estimate and every break of a cycle, which the GPU tests inspect before they compare.
"""
from __future__ import annotations

import numpy as np

from complex_oracle import SpMatMul, _Mem, addVectors, relax, solveCoarsest

GMRES_TOL = 1e-5                                 # MGcycle.jl:5


def julia_pinv(H):
    """Julia's pinv of the Hermitian H: SVD, singular values below eps * size * sigma_max dropped.  A Hermitian matrix whose
    imaginary part is exactly zero is real symmetric and goes through LAPACK's real driver, as the pinv of
    oracle/mg_oracle.py does (see FGMRES_relaxation on why the route matters)."""
    rcond = np.finfo(float).eps * min(H.shape)
    if not H.imag.any():
        return np.linalg.pinv(np.ascontiguousarray(H.real), rcond=rcond).astype(np.complex128)
    return np.linalg.pinv(H, rcond=rcond)


def _cmul(Mr, Mi, v):
    """(Mr + i Mi) v from four real products."""
    vr, vi = np.ascontiguousarray(v.real), np.ascontiguousarray(v.imag)
    return (Mr @ vr - Mi @ vi) + 1j * (Mr @ vi + Mi @ vr)


def FGMRES_relaxation(Afun, r0, x0, inner, prec, TOL, record=None):
    """FGMRES.jl:48-126 for one complex vector: x0 += Z t.  Returns (x0, rnorms); ``record`` (a list) receives
    (used, rnorms).

    The small dense algebra is written out in real and imaginary parts - Z and AZ are kept as two real arrays each, every
    complex product M'v, Mv or dot is four real ones - with the numpy calls of oracle/mg_oracle.py's FGMRES_relaxation
    (``AZ.T @ AZ[:, j]``, ``np.dot(AZ[:, j], r0)``, ``pinv(H) @ xi``, ``Z @ t``).  BLAS fixes no summation order for a complex gemv,
    and the K-cycle's H is ill-conditioned (its two directions are M r and M A M r with M A close to the identity: cond(H) up to
    1.4e5 on 8^3 cells), so t = pinv(H) xi carries a last-bit difference in H, xi or the SVD times cond(H).  Written this way a
    real operator with a real right-hand side gives the sums of the real oracle exactly, and the comparison of
    tests/test_complex_kcycle_host.py pins what it is meant to pin, the operation order of the two branches."""
    n = r0.size
    rnorm0 = np.linalg.norm(r0)                  # l.65
    r0r, r0i = np.ascontiguousarray(r0.real), np.ascontiguousarray(r0.imag)
    H = np.zeros((inner, inner), dtype=np.complex128)
    xi = np.zeros(inner, dtype=np.complex128)
    t = np.zeros(inner, dtype=np.complex128)
    Zr, Zi = np.zeros((n, inner)), np.zeros((n, inner))
    AZr, AZi = np.zeros((n, inner)), np.zeros((n, inner))
    w = None
    rnorms = []
    for j in range(inner):
        z = prec(r0) if j == 0 else prec(w)      # l.83-87
        Zr[:, j], Zi[:, j] = z.real, z.imag
        w = Afun(z)                              # l.91
        AZr[:, j], AZi[:, j] = w.real, w.imag
        t = (AZr.T @ AZr[:, j] + AZi.T @ AZi[:, j]) + 1j * (AZr.T @ AZi[:, j] - AZi.T @ AZr[:, j])        # gemv 'C'  (l.95)
        xi[j] = (np.dot(AZr[:, j], r0r) + np.dot(AZi[:, j], r0i)) + 1j * (np.dot(AZr[:, j], r0i) - np.dot(AZi[:, j], r0r))   # l.97
        H[:, j] = t                              # l.99
        H[j, :] = t.conj()                       # l.100
        H = 0.5 * H + 0.5 * H.conj().T           # l.101
        Pinv = julia_pinv(H)
        t = _cmul(np.ascontiguousarray(Pinv.real), np.ascontiguousarray(Pinv.imag), xi)                   # l.102
        Ht = _cmul(np.ascontiguousarray(H.real), np.ascontiguousarray(H.imag), t)
        rn = np.sqrt(abs((np.vdot(t, Ht) - 2.0 * np.vdot(t, xi) + rnorm0 ** 2).real))                     # l.104
        rnorms.append(float(rn))
        if rn < TOL:                             # l.114-117
            break
    if inner > 0:
        x0 += _cmul(Zr, Zi, t)                   # l.121-123
    if record is not None:
        record.append((len(rnorms), list(rnorms)))
    return x0, rnorms


def recursiveCycle(param, b, x, level, mem=None, cycleType=None, trace=None):
    """One cycle from `level` (1-based): MGcycle.jl:1-118 with the Jac-GMRES and K branches."""
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
    npresmth = param.relaxPre(level)
    npostsmth = param.relaxPost(level)
    gmres_relax = param.relaxType == "Jac-GMRES"
    MM = lambda xx: D * xx                       # l.36-38
    Afun = lambda z: A @ z                       # getAfun (SolveFuncs.jl:65-71)

    def note(kind, inner, rec):
        if trace is not None and rec:
            trace.append((kind, level, inner, rec[0][0], rec[0][1]))

    if gmres_relax:                              # l.48-50
        rec = []
        x = FGMRES_relaxation(Afun, r, x, npresmth, MM, GMRES_TOL, rec)[0]
        note("pre", npresmth, rec)
    else:
        x = relax(A, r, x, b, D, npresmth)       # l.54
    SpMatMul(-1.0, A, x, 0.0, r)                 # l.58
    addVectors(1.0, b, r)                        # l.60
    xc = mem.x[level]
    xc[...] = 0.0                                # l.63-64
    bc = mem.b[level]
    SpMatMul(1.0, R, r, 0.0, bc)                 # l.66
    if level == nlevels - 1:
        xc = solveCoarsest(param, bc, xc)        # l.67-69
    else:
        if cycleType == "K":                     # l.72-76
            Ac = As[level]

            def MMG(v):
                yz = np.zeros_like(v)            # yzK .= 0.0
                return recursiveCycle(param, v, yz, level + 1, mem, "K", trace).copy()

            rec = []
            xc = FGMRES_relaxation(lambda z: Ac @ z, bc.copy(), xc, 2, MMG, GMRES_TOL, rec)[0]
            note("K", 2, rec)
        else:
            xc = recursiveCycle(param, bc, xc, level + 1, mem, cycleType, trace)          # l.78
            if cycleType == "W":
                xc = recursiveCycle(param, bc, xc, level + 1, mem, "W", trace)            # l.79-80
            elif cycleType == "F":
                xc = recursiveCycle(param, bc, xc, level + 1, mem, "V", trace)            # l.81-84
    SpMatMul(1.0, P, xc, 1.0, x)                 # l.90
    r[...] = b                                   # l.92
    SpMatMul(-1.0, A, x, 1.0, r)                 # l.93
    if gmres_relax:                              # l.96-98
        rec = []
        x = FGMRES_relaxation(Afun, r, x, npostsmth, MM, GMRES_TOL, rec)[0]
        note("post", npostsmth, rec)
    else:
        x = relax(A, r, x, b, D, npostsmth)      # l.102
    return x


def solveMG(param, b, x, history=None, trace=None):
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
        x = recursiveCycle(param, b, x, 1, mem, None, trace)
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


def all_rn(trace):
    """Every residual estimate of a trace, flat."""
    return np.array([rn for rec in trace for rn in rec[4]])


def rn_clear_of_tol(trace, factor=4.0):
    """True when no recorded rn lies within `factor` of the break's tolerance: the break is then the same discrete decision for
    any computation that reproduces rn to a few digits."""
    rn = all_rn(trace)
    return bool(np.all((rn >= factor * GMRES_TOL) | (rn <= GMRES_TOL / factor)))
