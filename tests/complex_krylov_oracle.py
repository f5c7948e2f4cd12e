"""TEST INFRASTRUCTURE ONLY.  numpy restatement of KrylovMethods.bicgstb / fgmres for complex vectors, the checker of the
ComplexF64 device drivers (mg_bicgstab_CFP64 / mg_fgmres_CFP64).  Imports no device code of the package.

These are ``bicgstb`` and ``fgmres`` of oracle/mg_oracle.py (the published algorithms as solveBiCGSTAB_MG / solveGMRES_MG call them,
SolveFuncs.jl:85-133) with complex scalars and Julia's dot, ``dot(a, b) = sum conj(a_i) b_i`` (np.vdot); on real data they
reduce to the real ones (tests/test_complex_krylov_host.py pins that).  What changes for VAL = ComplexF64:

  * BiCGSTAB: rho = dot(rtld, r), alpha = rho / dot(rtld, v), omega = dot(t, s) / dot(t, t), beta = (rho / rho1)(alpha / omega);
    breakdown is rho == 0 or omega == 0 as complex numbers;
  * FGMRES: H[k,i] = dot(V_k, w), H[i+1,i] = ||w|| (real).  The rotation of column i has a complex cosine and a real sine:
    rr = sqrt(|a|^2 + b^2), c = a / rr, s = b / rr with a = H[i,i], b = H[i+1,i]; applied as t = conj(c) H[k] + s H[k+1];
    H[k+1] = -s H[k] + c H[k+1]; H[k] = t, and to the right-hand side as s_{i+1} = -s s_i; s_i = conj(c) s_i.  The estimate
    |s_{i+1}| / ||b|| does not depend on that choice of rotation.

The preconditioner is one cycle of tests/complex_oracle.py from x = 0.  ``case`` builds the shared cases C1, C2, C3: a
shifted-Laplacian hierarchy (damping 0.5) and a system operator of its own (damping 0.05 or 0)."""
from __future__ import annotations

import numpy as np

import complex_oracle as corc
from complex_cases import complex_rhs, helmholtz


def preconditioner(param):
    """M(v) = (z .= 0; recursiveCycle(param, v, z, 1); z)  (SolveFuncs.jl:59), complex."""
    mem = corc._Mem(param)

    def M(v):
        z = np.zeros(v.shape[0], dtype=np.complex128)
        return corc.recursiveCycle(param, np.asarray(v, dtype=np.complex128), z, 1, mem).copy()

    return M


def bicgstb(Afun, b, tol=1e-6, maxIter=100, M1=None, x=None):
    """Returns (x, flag, iterations, resvec); flags 0 / -1 / -2 / -3 / -9 as mg_bicgstab_FP64."""
    n = b.size
    bn = np.linalg.norm(b)
    if bn == 0:
        return np.zeros(n, dtype=np.complex128), -9, 0, np.array([0.0])
    x = np.zeros(n, dtype=np.complex128) if x is None else np.array(x, dtype=np.complex128)
    r = b - Afun(x)
    M = M1 if M1 is not None else (lambda v: v.copy())
    resvec = [np.linalg.norm(r) / bn]
    if resvec[0] < tol:
        return x, 0, 0, np.array(resvec)
    rtld = r.copy()
    omega, alpha, rho1 = 1.0 + 0.0j, 0.0j, 0.0j
    p = np.zeros(n, dtype=np.complex128)
    v = np.zeros(n, dtype=np.complex128)
    flag, it = -1, 0
    for k in range(1, maxIter + 1):
        it = k
        rho = np.vdot(rtld, r)
        if rho == 0.0:
            flag = -2
            break
        if k > 1:
            beta = (rho / rho1) * (alpha / omega)
            p = r + beta * (p - omega * v)
        else:
            p = r.copy()
        phat = M(p)
        v = Afun(phat)
        alpha = rho / np.vdot(rtld, v)
        s = r - alpha * v
        sn = np.linalg.norm(s) / bn
        resvec.append(sn)
        if sn < tol:
            x = x + alpha * phat
            flag = -3
            break
        shat = M(s)
        t = Afun(shat)
        omega = np.vdot(t, s) / np.vdot(t, t).real
        x = x + (alpha * phat + omega * shat)
        r = s - omega * t
        err = np.linalg.norm(r) / bn
        resvec.append(err)
        if err <= tol:
            flag = 0
            break
        if omega == 0.0:
            flag = -2
            break
        rho1 = rho
    return x, flag, it, np.array(resvec)


def fgmres(Afun, b, restrt, tol=1e-2, maxIter=100, M=None, x=None):
    """Returns (x, flag, total inner steps, resvec); maxIter counts restarts."""
    n = b.size
    bn = np.linalg.norm(b)
    if bn == 0:
        return np.zeros(n, dtype=np.complex128), -9, 0, np.zeros(0)
    x = np.zeros(n, dtype=np.complex128) if x is None else np.array(x, dtype=np.complex128)
    Mf = M if M is not None else (lambda v: v.copy())
    r = b - Afun(x)
    rn = np.linalg.norm(r)
    if rn / bn < tol:
        return x, 0, 0, np.zeros(0)
    m = restrt
    resvec, flag, total = [], -1, 0
    for it in range(1, maxIter + 1):
        V = np.zeros((n, m + 1), dtype=np.complex128)
        Z = np.zeros((n, m), dtype=np.complex128)
        H = np.zeros((m + 1, m), dtype=np.complex128)
        cs = np.zeros(m, dtype=np.complex128)
        sn = np.zeros(m)
        s = np.zeros(m + 1, dtype=np.complex128)
        V[:, 0] = r / rn
        s[0] = rn
        used = 0
        for i in range(m):
            Z[:, i] = Mf(V[:, i].copy())
            w = Afun(Z[:, i])
            for k in range(i + 1):
                H[k, i] = np.vdot(V[:, k], w)
                w = w - H[k, i] * V[:, k]
            wn = np.linalg.norm(w)
            H[i + 1, i] = wn
            if wn != 0:
                V[:, i + 1] = w / wn
            for k in range(i):
                t = np.conj(cs[k]) * H[k, i] + sn[k] * H[k + 1, i]
                H[k + 1, i] = -sn[k] * H[k, i] + cs[k] * H[k + 1, i]
                H[k, i] = t
            a = H[i, i]
            rr = np.sqrt(a.real * a.real + a.imag * a.imag + wn * wn)
            cs[i], sn[i] = (1.0, 0.0) if rr == 0 else (a / rr, wn / rr)
            H[i, i], H[i + 1, i] = rr, 0.0
            s[i + 1] = -sn[i] * s[i]
            s[i] = np.conj(cs[i]) * s[i]
            err = abs(s[i + 1]) / bn
            resvec.append(err)
            total += 1
            used = i + 1
            if err <= tol:
                flag = 0
                break
        y = np.zeros(used, dtype=np.complex128)
        for i in range(used - 1, -1, -1):                     # y = H \ s, back substitution
            y[i] = (s[i] - H[i, i + 1:used] @ y[i + 1:used]) / H[i, i]
        x = x + Z[:, :used] @ y
        if flag == 0:
            break
        r = b - Afun(x)
        rn = np.linalg.norm(r)
        if rn / bn <= tol:
            flag = 0
            break
    return x, flag, total, np.array(resvec)


# ---- the shared cases -----------------------------------------------------------------------------------------------------------
TOL = 1e-8
MAXIT_BICGSTAB = 40          # iterations
MAXIT_FGMRES = 20            # restarts
#        cells, levels, damping of the system operator
CASES = {"C1": (16, 3, 0.05), "C2": (16, 3, 0.0), "C3": (8, 2, 0.05)}
# what the oracle takes on them (tests/test_complex_krylov_host.py asserts these): BiCGSTAB (iterations, flag); FGMRES steps by `inner`
EXPECTED = {"C1": {"bicgstab": (19, -3), 5: 57, 10: 45},
            "C2": {"bicgstab": (27, 0), 10: 67},
            "C3": {"bicgstab": (11, -3), 5: 43, 10: 22}}

_cache = {}


def case(mg, name):
    """(param, A_sys, b): k h = 0.5, the hierarchy (SPAI, V(2,1)) on the operator with damping 0.5, the system operator with the
    case's damping, b = complex_rhs(n, 21).  Built once per process and shared - nothing in it may be modified."""
    if name not in _cache:
        cells, levels, damp = CASES[name]
        Ah, mesh = helmholtz(mg, [cells] * 3, 0.5, 0.5)
        p = mg.getMGparam(np.complex128, np.int64, levels, 8, MAXIT_BICGSTAB, TOL, "SPAI", 1.0, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
        mg.MGsetup(Ah, mesh, p)
        As, _ = helmholtz(mg, [cells] * 3, 0.5, damp)
        _cache[name] = (p, As, complex_rhs(Ah.shape[0], 21))
    return _cache[name]


_runs = {}


def reference(mg, name, method, inner=None, x0=None, maxIter=None, key=None):
    """The oracle's run of a case, computed once and shared: (x, flag, count, resvec).  key: a name for a variant (x0 / maxIter given)."""
    k = (name, method, inner, key)
    if k not in _runs:
        p, As, b = case(mg, name)
        Afun = lambda v: As @ v
        M = preconditioner(p)
        if method == "bicgstab":
            _runs[k] = bicgstb(Afun, b, TOL, MAXIT_BICGSTAB if maxIter is None else maxIter, M, x0)
        else:
            _runs[k] = fgmres(Afun, b, inner, TOL, MAXIT_FGMRES if maxIter is None else maxIter, M, x0)
    return _runs[k]
