"""Shared by the complex Vanka tests: the cases (mixed elastic Helmholtz operators of tests/vanka_cases.py, damping 0.1), their
hierarchies through MGsetup with ``complexVanka=True``, and the numpy restatement of the cycle with Vanka relaxation - the
V / W recursion of ``vanka_cases.restate_vcycle`` written once more with the F and K branches of MGcycle.jl:72-84 (the K branch:
two ``complex_kcycle_oracle.FGMRES_relaxation`` steps on a level below which another non-coarsest level lies, preconditioned by
the same recursion from zero).  Dtype-generic: complex128, and complex64 with the coarsest solve in double on the widened
operator, as the package does.  Imports no device code of the package."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import vanka_cases as V
from complex_kcycle_oracle import GMRES_TOL, FGMRES_relaxation, _cmul, julia_pinv

W, MASS = 0.6, 1e-2
# name -> (cells, levels, omega, cycle); V(1,1), w = 0.6, lam = mu = 1, mass = 1e-2.  Residual factors of the restatement over 5
# cycles (asserted < 0.5 by tests/test_complex_vanka_host.py::test_restatement_contracts): 32v 0.135 0.213 0.237 0.289 0.356;
# 32w 0.132 0.209 0.217 0.231 0.267; 32k 0.132 0.208 0.215 0.225 0.254; 24v 0.140 0.210 0.222 0.245 0.289; 24w 0.137 0.208 0.214
# 0.221 0.242; 12v 0.143 0.241 0.283 0.321 0.350; 16v 0.140 0.237 0.277 0.321 0.365.  omega is not to be raised: 0.2 on [32,32]
# gives V factors up to 0.53 and 0.4 diverges.  The non-cubic boxes are there because the index arithmetic mixes n1, n2, n3;
# [12,8,10] has 120 cells per colour (3.75 workgroups: the partial group runs); level 2 of [24,16] has 24 cells per colour.
CASES = {
    "32v": ([32, 32], 3, 0.15, "V"),
    "32w": ([32, 32], 3, 0.15, "W"),
    "32k": ([32, 32], 3, 0.15, "K"),
    "24v": ([24, 16], 3, 0.15, "V"),
    "24w": ([24, 16], 3, 0.15, "W"),
    "12v": ([12, 8, 10], 2, 0.3, "V"),
    "16v": ([16, 16, 16], 2, 0.3, "V"),
}
VTYPES = {"VankaFaces": V.FULL_VANKA_RB, "EconVankaFaces": V.ECON_VANKA_RB, "VankaFacesAdd": V.FULL_VANKA_ADD}

_ops, _params = {}, {}


def operator(n, omega):
    key = (tuple(n), omega)
    if key not in _ops:
        _ops[key] = V.mixed_operator(n, True, omega=omega, mass=MASS)
    return _ops[key]


def mesh(mg, n):
    return mg.getRegularMesh([0, 1] * len(n), n)


def rhs(N, single=False):
    b = V.seeded(N, 5, cx=True)
    return b.astype(np.complex64) if single else b


def param(mg, name, single=False, relaxType="VankaFaces", w=W, cycle=None, maxIter=5, tol=1e-30):
    """The case's hierarchy through MGsetup (cached: the tests read it, the device handle stays with it)."""
    n, levels, omega, cyc = CASES[name]
    cyc = cycle or cyc
    key = (name, single, relaxType, w, cyc, maxIter, tol)
    if key not in _params:
        p = mg.getMGparam(np.complex128, np.int64, levels, 1, maxIter, tol, relaxType, w, 1, 1, cyc, "NoMUMPS", 0.4, 0.0,
                          "SystemsFacesMixedLinear", singlePrecision=single, complexVanka=True)
        mg.MGsetup(operator(n, omega), mesh(mg, n), p)
        assert p.levels == levels
        _params[key] = p
    return _params[key]


class CoarseLU:
    """z = LU \\ b in double on the operator widened, the result in b's type (MGsetup.jl:350 for a ComplexF32 hierarchy)."""

    def __init__(self, Ac):
        self.lu = spla.splu(sp.csc_matrix(Ac).astype(np.complex128))

    def solve(self, b):
        return self.lu.solve(b.astype(np.complex128)).astype(b.dtype)


class Hier:
    """What the restatement reads of a param.  widen: a ComplexF32 param's operators as complex128 / float64 with the SAME
    (rounded) values - the comparand of the single-precision tests."""

    def __init__(self, p, widen=False):
        cd, rd = (np.complex128, np.float64) if widen else (p.As[0].dtype, p.Ps[0].dtype)
        self.As = [sp.csr_matrix(A, dtype=cd) for A in p.As]
        self.Ps = [sp.csr_matrix(P, dtype=rd) for P in p.Ps]
        self.Rs = [sp.csr_matrix(R, dtype=rd) for R in p.Rs]
        self.Ds = list(p.relaxPrecs)
        self.ns = [list(map(int, m.n)) for m in p.Meshes]
        self.ip = p.transferOperatorType == "SystemsFacesMixedLinear"
        self.vtype = VTYPES[p.relaxType]
        self.lu = CoarseLU(self.As[-1])
        self.npre, self.npost = p.relaxPre(1), p.relaxPost(1)
        self.dtype = np.dtype(cd)


def FGMRES_relaxation_ld(Afun, r0, x0, inner, prec, TOL, record=None):
    """complex_kcycle_oracle.FGMRES_relaxation with the dots (column j of H, xi[j], norm(r0)) summed in np.longdouble and rounded
    once; everything else as there.  The distance of a cycle run with it from the plain run measures what the summation order of
    those dots can move."""
    ld = np.longdouble
    n = r0.size
    r0r, r0i = r0.real.astype(ld), r0.imag.astype(ld)
    rnorm0 = float(np.sqrt(np.dot(r0r, r0r) + np.dot(r0i, r0i)))
    H = np.zeros((inner, inner), dtype=np.complex128)
    xi = np.zeros(inner, dtype=np.complex128)
    t = np.zeros(inner, dtype=np.complex128)
    Zr, Zi = np.zeros((n, inner)), np.zeros((n, inner))
    AZr, AZi = np.zeros((n, inner), dtype=ld), np.zeros((n, inner), dtype=ld)
    w = None
    rnorms = []
    for j in range(inner):
        z = prec(r0) if j == 0 else prec(w)
        Zr[:, j], Zi[:, j] = z.real, z.imag
        w = Afun(z)
        AZr[:, j], AZi[:, j] = w.real, w.imag
        tr = AZr.T @ AZr[:, j] + AZi.T @ AZi[:, j]
        ti = AZr.T @ AZi[:, j] - AZi.T @ AZr[:, j]
        t = tr.astype(np.float64) + 1j * ti.astype(np.float64)
        xi[j] = float(np.dot(AZr[:, j], r0r) + np.dot(AZi[:, j], r0i)) + 1j * float(np.dot(AZr[:, j], r0i) - np.dot(AZi[:, j], r0r))
        H[:, j] = t
        H[j, :] = t.conj()
        H = 0.5 * H + 0.5 * H.conj().T
        Pinv = julia_pinv(H)
        t = _cmul(np.ascontiguousarray(Pinv.real), np.ascontiguousarray(Pinv.imag), xi)
        Ht = _cmul(np.ascontiguousarray(H.real), np.ascontiguousarray(H.imag), t)
        rn = np.sqrt(abs((np.vdot(t, Ht) - 2.0 * np.vdot(t, xi) + rnorm0 ** 2).real))
        rnorms.append(float(rn))
        if rn < TOL:
            break
    if inner > 0:
        x0 += _cmul(Zr, Zi, t)
    if record is not None:
        record.append((len(rnorms), list(rnorms)))
    return x0, rnorms


def restate_cycle(H, b, x, x_zero, cycle, level=0, fgmres=FGMRES_relaxation, trace=None):
    """recursiveCycle (MGcycle.jl:1-118) with Vanka relaxation on every non-coarsest level: ``vanka_cases.restate_vcycle`` with the
    F branch (l.81-84) and the K branch (l.72-76).  ``trace`` receives the K steps' records in the format of complex_kcycle_oracle."""
    nl = len(H.As)
    if level == nl - 1:
        return H.lu.solve(b)
    A = H.As[level]
    if x_zero:
        x = np.zeros_like(b)
    x = V.restate_relax(A, x.copy(), b, H.Ds[level], H.npre, H.ns[level], H.ip, H.vtype)
    r = b - A @ x
    bc = H.Rs[level] @ r
    if level + 1 == nl - 1:
        xc = H.lu.solve(bc)
    elif cycle == "K":
        Ac = H.As[level + 1]
        rec = []
        xc = fgmres(lambda z: Ac @ z, bc.copy(), np.zeros_like(bc), 2,
                    lambda v: restate_cycle(H, v, None, True, "K", level + 1, fgmres, trace), GMRES_TOL, rec)[0]
        if trace is not None:
            trace.append(("K", level + 1, 2, rec[0][0], rec[0][1]))
    else:
        xc = restate_cycle(H, bc, None, True, cycle, level + 1, fgmres, trace)
        if cycle == "W":
            xc = restate_cycle(H, bc, xc, False, "W", level + 1, fgmres, trace)
        elif cycle == "F":
            xc = restate_cycle(H, bc, xc, False, "V", level + 1, fgmres, trace)
    x = x + H.Ps[level] @ xc
    return V.restate_relax(A, x, b, H.Ds[level], H.npost, H.ns[level], H.ip, H.vtype)


def restate_history(H, b, cycles, cycle, fgmres=FGMRES_relaxation, trace=None):
    """solveMG's loop from x = 0: ([x after each cycle], [||r_0||, ||r_1||, ...])."""
    x = np.zeros_like(b)
    xs, res = [], [np.linalg.norm(b)]
    for it in range(cycles):
        x = restate_cycle(H, b, x, it == 0, cycle, 0, fgmres, trace)
        xs.append(x.copy())
        res.append(np.linalg.norm(b - H.As[0] @ x))
    return xs, np.array(res)


_runs = {}


def reference(mg, name, cycles=2, **kw):
    """(param, Hier, b, [x after each cycle], residual history, trace) of a case's complex128 restatement, computed once per
    (case, cycles, options) and left unchanged."""
    key = (name, cycles, tuple(sorted(kw.items())))
    if key not in _runs:
        p = param(mg, name, **kw)
        H = Hier(p)
        b = rhs(p.As[0].shape[0])
        trace = []
        xs, res = restate_history(H, b, cycles, p.cycleType, trace=trace)
        for a in xs + [res, b]:
            a.setflags(write=False)
        _runs[key] = (p, H, b, xs, res, trace)
    return _runs[key]


def err_max(a, ref):
    return np.abs(a - ref).max() / np.abs(ref).max()


def rel2(a, ref):
    return np.linalg.norm(a - ref) / np.linalg.norm(ref)
