"""Shared by tests/test_complex_single_kcycle_host.py and tests/test_complex_single_kcycle_gpu.py: the operators, hierarchies and
oracle runs of the ``singleKcycle`` tests, computed once per process and never modified.  Imports no device code of the package.

The relaxation cases are the operators of tests/test_complex_kcycle_gpu.py (generators copied) with values rounded to complex64 and
|d| ~ 0.1.  The cycle cases are Helmholtz on 16^3 cells with 3 and 4 levels (its PROBLEMS and SCHEDULES), set up with
``singlePrecision=True, singleKcycle=True``; for each the complex128 oracle (complex_kcycle_oracle on ``rounded(param)``), the single
oracle (complex_single_kcycle_oracle) and both traces."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import complex_coarse_cases as ccase
import complex_kcycle_oracle as korc
import complex_single_kcycle_oracle as sk
import complex_vanka_cases as vcase
from complex_cases import complex_rhs, helmholtz

C64 = np.complex64
C128 = np.complex128
U32 = 2.0 ** -24
INNERS = (1, 3, 8)


def single_param(mg, levels, relax, omega, pre, post, cyc, maxIter=5, tol=1e-10, coarse="NoMUMPS", **kw):
    return mg.getMGparam(np.complex128, np.int64, levels, 8, maxIter, tol, relax, omega, pre, post, cyc, coarse, 0.5, 0.0,
                         singlePrecision=True, singleKcycle=True, **kw)


# ---- the relaxation cases -------------------------------------------------------------------------------------------------------------
def _awkward_operator(n, seed):
    """Complex square CSR with empty rows, rows spanning the kernel's 1024-entry chunks and one row longer than a chunk (row 2000:
    3000 entries, the branch in which the whole workgroup strides over one row); values rounded to complex64."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 12, n)
    lens[rng.choice(n, 40, replace=False)] = 0
    lens[100:104] = [700, 650, 900, 400]
    lens[2000] = 3000
    rows, cols = [], []
    for i, k in enumerate(lens):
        c = np.sort(rng.choice(n, int(k), replace=False))
        rows.append(np.full(len(c), i))
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = (rng.standard_normal(len(rows)) + 1j * rng.standard_normal(len(rows))).astype(C64)
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    A.sort_indices()
    return A


def _small_operator(n, seed):
    """n <= 256 rows and fewer than 1024 entries: a level of ONE row block; values rounded to complex64."""
    A = (sp.random(n, n, density=3.0 / n, random_state=seed) + 1j * sp.random(n, n, density=3.0 / n, random_state=seed + 1)
         + sp.identity(n) * (3.0 + 1.0j)).tocsr().astype(C64)
    A.sort_indices()
    assert A.nnz < 1024
    return A


def _manual_param(mg, A, nc, seed):
    """A two-level ComplexF32 param around an arbitrary A (float32 random P and R, a complex64 coarse operator), |d| ~ 0.1."""
    rng = np.random.default_rng(seed)
    n = A.shape[0]
    P = sp.random(n, nc, density=4.0 / nc, random_state=seed, format="csr").astype(np.float32)
    R = sp.random(nc, n, density=6.0 / n, random_state=seed + 1, format="csr").astype(np.float32)
    P.sort_indices()
    R.sort_indices()
    Ac = (sp.identity(nc) * (4.0 + 1j) + 0.1 * sp.random(nc, nc, density=0.05, random_state=seed + 2)).tocsr().astype(C64)
    Ac.sort_indices()
    p = single_param(mg, 2, "Jac", 0.8, 1, 1, "V", 4, 1e-6)
    p.As, p.Ps, p.Rs = [A, Ac], [P], [R]
    p.relaxPrecs = [(0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(C64)]
    p.LU = spla.splu(sp.csc_matrix(Ac.astype(C128)))
    p.nrhs = 1
    return p


_OPS = {"awkward5000": lambda: (_awkward_operator(5000, 3), 700), "oneblock100": lambda: (_small_operator(100, 5), 20)}
_relax = {}


def relax_param(mg, name):
    if name not in _relax:
        A, nc = _OPS[name]()
        _relax[name] = _manual_param(mg, A, nc, 7)
    return _relax[name]


def relax_vectors(n):
    """(r0, x0) of the relaxation cases, complex64."""
    return complex_rhs(n, 31).astype(C64), complex_rhs(n, 32).astype(C64)


_relax_runs = {}


def relax_reference(mg, name, inner, scale=1.0):
    """The single oracle's relaxation on a relaxation case: dict(x, rnorms, H, xi, Z, AZ, cond), computed once."""
    key = (name, inner, scale)
    if key not in _relax_runs:
        p = relax_param(mg, name)
        A, d = p.As[0], p.relaxPrecs[0]
        r0, x0 = relax_vectors(A.shape[0])
        r0 = (scale * r0.astype(C128)).astype(C64)
        if scale != 1.0:
            x0 = np.zeros_like(x0)
        bases = {}
        x, rn = sk.FGMRES_relaxation(sk._spmv(A), r0, x0.copy(), inner, lambda v: d * v, 1e-5, None, bases)
        _relax_runs[key] = dict(x=x, rnorms=rn, r0=r0, x0=x0, cond=float(np.linalg.cond(bases["H"])), **bases)
    return _relax_runs[key]


# ---- the cycle cases --------------------------------------------------------------------------------------------------------------------
PROBLEMS = {"3lev": ([16, 16, 16], 0.5, 3), "4lev": ([16, 16, 16], 0.25, 4)}
SCHEDULES = [("Jac-GMRES", "V", 2, 2), ("Jac-GMRES", "K", 2, 1), ("Jac", "K", 2, 1), ("SPAI", "K", 2, 1), ("Jac-GMRES", "K", 1, 1)]
# (problem, schedule, variant): "zero" from x = 0; "second" from the single oracle's first iterate; "gmres" with coarseSolveType
# "GMRES"; "vanka" the complex Vanka K(1,1) hierarchy on the grid of complex_vanka_cases' "32k"
CYCLE_CASES = [(prob, s, "zero") for prob in ("3lev", "4lev") for s in SCHEDULES] + [
    ("4lev", ("Jac-GMRES", "K", 2, 1), "second"), ("3lev", ("Jac-GMRES", "K", 2, 1), "gmres"), ("32k", ("VankaFaces", "K", 1, 1), "vanka")]


def case_id(v):
    return "-".join(map(str, v)) if isinstance(v, tuple) else str(v)


def helm_param(mg, prob, sched, maxIter=5, tol=1e-10, damping=0.5, coarse="NoMUMPS", **kw):
    cells, kh, levels = PROBLEMS[prob]
    A, mesh = helmholtz(mg, cells, kh, damping)
    relax, cyc, pre, post = sched
    p = single_param(mg, levels, relax, 0.8, pre, post, cyc, maxIter, tol, coarse, **kw)
    mg.MGsetup(A, mesh, p)
    return p


def vanka_param(mg, name="32k"):
    n, levels, omega, cyc = vcase.CASES[name]
    p = mg.getMGparam(np.complex128, np.int64, levels, 1, 5, 1e-30, "VankaFaces", vcase.W, 1, 1, cyc, "NoMUMPS", 0.4, 0.0,
                      "SystemsFacesMixedLinear", singlePrecision=True, complexVanka=True, singleKcycle=True)
    mg.MGsetup(vcase.operator(n, omega), vcase.mesh(mg, n), p)
    return p


def cycle_oracles(p, b, x0, trace64=None, traces=None):
    """(x64, xs): one cycle of complex_kcycle_oracle on rounded(p) and of the single oracle on p, from the complex64 x0."""
    x64 = korc.recursiveCycle(sk.rounded(p), b.astype(C128), x0.astype(C128), 1, trace=trace64).copy()
    xs = sk.recursiveCycle(p, b, x0.copy(), 1, trace=traces).copy()
    return x64, xs


def dist(x, x64):
    return float(np.abs(np.asarray(x, dtype=C128) - x64).max() / np.abs(x64).max())


_cycle = {}


def cycle_reference(mg, prob, sched, variant):
    """dict(p, po, b, x0, x64, xs, trace64, traces, e_ref) of a cycle case: p the param the device takes, po the param the oracles
    read (p itself, or p with the oracle's GMRES coarsest solve in LU)."""
    key = (prob, sched, variant)
    if key in _cycle:
        return _cycle[key]
    t64, ts = [], []
    if variant == "vanka":
        p = po = vanka_param(mg, prob)
        b = vcase.rhs(p.As[0].shape[0], single=True)
        x0 = np.zeros_like(b)
        x64 = vcase.restate_cycle(vcase.Hier(p, widen=True), b.astype(C128), None, True, "K", trace=t64)
        xs = vcase.restate_cycle(vcase.Hier(p), b, None, True, "K", fgmres=sk.FGMRES_relaxation, trace=ts)
        assert xs.dtype == C64
    else:
        p = helm_param(mg, prob, sched, coarse="GMRES" if variant == "gmres" else "NoMUMPS")
        po = ccase.oracle_param(p) if variant == "gmres" else p
        b = complex_rhs(p.As[0].shape[0], 9).astype(C64)
        x0 = np.zeros_like(b)
        if variant == "second":
            x0 = sk.recursiveCycle(po, b, x0, 1).copy()
        x64, xs = cycle_oracles(po, b, x0, t64, ts)
    _cycle[key] = dict(p=p, po=po, b=b, x0=x0, x64=x64, xs=xs, trace64=t64, traces=ts, e_ref=dist(xs, x64))
    return _cycle[key]


def used(trace):
    return [(rec[0], rec[1], rec[2], rec[3]) for rec in trace]


# ---- solveMG and the drivers ------------------------------------------------------------------------------------------------------------
SOLVE_SCHED = ("Jac", "K", 2, 1)
# b is scaled by 1e3 so that every residual estimate of the solve's cycles stays a factor 4 or more above the break's 1e-5 on the oracle
# (with |b| ~ 1 the K steps of the last cycles come down to 3.6e-6); the tolerance 1e-4 is met after 8 cycles with the residual
# a factor 1.6 away from it on either side
SOLVE_SCALE = 1e3
_solve = {}


def solve_reference(mg):
    """The single oracle's solveMG on the 3-level K(2,1) Jac case: dict(p, b, x, iters, resvec, trace, trace64, iters64, e_ref); e_ref
    is the relative 2-norm distance of one single cycle from the double one (what tests/test_complex_single_gpu.py scales its resvec
    bound by); trace64 / iters64 are the double oracle's solve on rounded(p)."""
    if not _solve:
        import complex_single_oracle as cs
        p = helm_param(mg, "3lev", SOLVE_SCHED, maxIter=12, tol=1e-4)
        b = (SOLVE_SCALE * complex_rhs(p.As[0].shape[0], 12)).astype(C64)
        hist, trace = {}, []
        x, it = sk.solveMG(p, b, np.zeros_like(b), hist, trace)
        x64, xs = cycle_oracles(p, b, np.zeros_like(b))
        trace64 = []
        _, it64 = korc.solveMG(sk.rounded(p), b.astype(C128), np.zeros(b.shape[0], dtype=C128), None, trace64)
        _solve.update(p=p, b=b, x=x.copy(), iters=it, resvec=hist["resvec"], trace=trace, trace64=trace64, iters64=it64,
                      e_ref=cs.rel2(xs, x64))
    return _solve


DRIVER_SCHEDS = {"K21jac": ("Jac", "K", 2, 1), "V22jacgmres": ("Jac-GMRES", "V", 2, 2)}
# The right-hand side's seed per hierarchy: chosen ON THE ORACLE so that its BiCGSTAB ends at a full step (flag 0) with the half step
# before it 10% or more above the tolerance and the last residual 10% or more below (asserted by the GPU test before it compares) -
# where BiCGSTAB ends is a discrete decision, and with seed 21 of the ComplexF64 test the oracle itself ends at a half step (flag -3).
DRIVER_SEED = {"K21jac": 26, "V22jacgmres": 29}
DRIVER_SCALE = 1e6
FGMRES_INNER = 5
_drivers = {}


def driver_reference(mg, name):
    """The complex128 oracle drivers on the nearly undamped operator (damping 0.05), preconditioned by the single oracle through the
    mixed closure: dict(p, As, b, bicgstab, fgmres, bicgstab_double_count, traces, traces64), each run (x, flag, count, resvec);
    traces / traces64: the relaxations' records of the (BiCGSTAB, FGMRES) runs with the single and with the double oracle as M."""
    if name not in _drivers:
        import complex_krylov_oracle as ck
        cells, kh, _ = PROBLEMS["4lev"]
        As, _ = helmholtz(mg, cells, kh, 0.05)
        p = helm_param(mg, "4lev", DRIVER_SCHEDS[name], maxIter=ck.MAXIT_BICGSTAB, tol=ck.TOL)
        b = DRIVER_SCALE * complex_rhs(As.shape[0], DRIVER_SEED[name])
        Afun = lambda v: As @ v
        tb, tg = [], []
        bic = ck.bicgstb(Afun, b, ck.TOL, ck.MAXIT_BICGSTAB, preconditioner_of(p, tb))
        fg = ck.fgmres(Afun, b, FGMRES_INNER, ck.TOL, ck.MAXIT_FGMRES, preconditioner_of(p, tg))
        pr = sk.rounded(p)
        mem = korc._Mem(pr)
        tb64, tg64 = [], []
        M64 = lambda tr: (lambda v: korc.recursiveCycle(pr, np.asarray(v, dtype=C128), np.zeros(v.shape[0], dtype=C128), 1, mem, None, tr).copy())
        bic64 = ck.bicgstb(Afun, b, ck.TOL, ck.MAXIT_BICGSTAB, M64(tb64))
        ck.fgmres(Afun, b, FGMRES_INNER, ck.TOL, ck.MAXIT_FGMRES, M64(tg64))
        _drivers[name] = dict(p=p, As=As, b=b, bicgstab=bic, fgmres=fg, bicgstab_double_count=bic64[2], traces=(tb, tg), traces64=(tb64, tg64))
    return _drivers[name]


def preconditioner_of(p, trace):
    return sk.preconditioner(p, trace)
