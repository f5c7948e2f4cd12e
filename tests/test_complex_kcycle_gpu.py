"""-m gpu: ComplexF64 Jac-GMRES smoothing and the K-cycle on the MI355X (mg_set_schedule_CF64, mg_fgmres_relax_CF64, the GRAM
epilogue of cx_csr_stream_spmv) against numpy and tests/complex_kcycle_oracle.py on the same host-built hierarchy.

Tolerances.
  * Gram scalars (H = AZ'AZ, xi = AZ'r0), row by row: 1e-12 of the largest entry - sums of <= 5000 products of O(1) numbers, any
    order: n * eps = 1e-12 would be the worst case, the usual sqrt(n) * eps = 2e-14.
  * x of one relaxation: 100 * eps * cond(H) relative; the test computes cond(H) from the oracle's H and asserts cond(H) <= 1e8
    (d is scaled by 0.1 for that: with |d| ~ 1 the directions of this operator grow by 10 per step and cond(H) is 3e10 for 8).
  * Cycles: 1e-11 of max|x|.  Measured on the CPU with the dots in extended precision instead of double: these cycles moved by
    at most 9.5e-14 at cond(H) up to 5.9e4 - a margin of 100.
  * The break at rn < 1e-5 is a discrete decision.  Every test that compares a cycle first asserts ON THE ORACLE'S rn ALONE that
    none lies within a factor 4 of 1e-5; if that fails the input is wrong (change b's scale, never the factor).  Closest here: a
    factor 4.5 (Jac K(2,1), four levels).
  * solveMG: resvec within 1e-10 * resvec[0]; drivers: the bounds of tests/test_complex_krylov_gpu.py (1e-8)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import complex_krylov_oracle as ck
import complex_kcycle_oracle as korc
from complex_cases import complex_rhs, helmholtz

pytestmark = pytest.mark.gpu

MG_ERR_INVALID, MG_ERR_STATE, MG_ERR_UNSUPPORTED = 1, 3, 4
EPS = np.finfo(float).eps
_dp = C.POINTER(C.c_double)
dz = lambda a: a.ctypes.data_as(_dp)


# ---- the kernel, row by row ---------------------------------------------------------------------------------------------------------
def _awkward_operator(n, seed):
    """Complex square CSR with empty rows, rows spanning the kernel's 1024-entry chunks and one row longer than a chunk (row 2000:
    3000 entries, the branch in which the whole workgroup strides over one row)."""
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
    vals = rng.standard_normal(len(rows)) + 1j * rng.standard_normal(len(rows))
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    A.sort_indices()
    return A


def _small_operator(n, seed):
    """n <= 256 rows and fewer than 1024 entries: a level of ONE row block."""
    A = (sp.random(n, n, density=3.0 / n, random_state=seed) + 1j * sp.random(n, n, density=3.0 / n, random_state=seed + 1)
         + sp.identity(n) * (3.0 + 1.0j)).tocsr()
    A.sort_indices()
    assert A.nnz < 1024
    return A


def _manual_param(mg, A, nc, seed):
    """A two-level complex param around an arbitrary A (as tests/test_complex_gpu.py's), with |d| ~ 0.1."""
    rng = np.random.default_rng(seed)
    n = A.shape[0]
    P = sp.random(n, nc, density=4.0 / nc, random_state=seed, format="csr")
    R = sp.random(nc, n, density=6.0 / n, random_state=seed + 1, format="csr")
    P.sort_indices()
    R.sort_indices()
    Ac = (sp.identity(nc) * (4.0 + 1j) + 0.1 * sp.random(nc, nc, density=0.05, random_state=seed + 2)).tocsr().astype(np.complex128)
    Ac.sort_indices()
    p = mg.getMGparam(np.complex128, np.int64, 2, 8, 4, 1e-10, "Jac", 0.8, 1, 1, "V")
    p.As, p.Ps, p.Rs = [A, Ac], [P], [R]
    p.relaxPrecs = [0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))]
    p.LU = spla.splu(sp.csc_matrix(Ac))
    p.nrhs = 1
    return p


_OPS = {"awkward5000": lambda: (_awkward_operator(5000, 3), 700), "oneblock100": lambda: (_small_operator(100, 5), 20)}
_kernel_cache = {}


def _kernel_case(mg, name):
    if name not in _kernel_cache:
        A, nc = _OPS[name]()
        p = _manual_param(mg, A, nc, 7)
        _kernel_cache[name] = (p, mg.device.DeviceHierarchy(p))
    return _kernel_cache[name]


@pytest.fixture(scope="module", autouse=True)
def _close_kernel_cases():
    yield
    for _, dev in _kernel_cache.values():
        dev.close()
    _kernel_cache.clear()


@pytest.mark.parametrize("inner", [1, 3, 8])
@pytest.mark.parametrize("name", ["awkward5000", "oneblock100"])
def test_gram_kernel_row_by_row(mg, built, name, inner):
    p, dev = _kernel_case(mg, name)
    A, d = p.As[0], p.relaxPrecs[0]
    n = A.shape[0]
    assert n % 256 != 0
    r0 = complex_rhs(n, 31)
    x0 = complex_rhs(n, 32)
    if name == "awkward5000":
        assert A.indptr[2001] - A.indptr[2000] == 3000 and d[2000] != 0 and r0[2000] != 0     # the long row feeds every partial
    Z = np.zeros((n, inner), dtype=np.complex128)
    AZ = np.zeros((n, inner), dtype=np.complex128)
    z = d * r0
    for j in range(inner):
        Z[:, j] = z
        AZ[:, j] = A @ z
        z = d * AZ[:, j]
    Href, xiref = AZ.conj().T @ AZ, AZ.conj().T @ r0
    cond = np.linalg.cond(Href)
    assert cond <= 1e8
    xo, rno = korc.FGMRES_relaxation(lambda v: A @ v, r0, x0.copy(), inner, lambda v: d * v, 1e-5)
    assert len(rno) == inner and min(rno) > 4e-5                 # no break in this case: every direction is used
    x = x0.copy()
    rn, H, xi = dev.fgmres_relax(1, r0, x, inner)
    eh = np.abs(H - Href).max() / np.abs(Href).max()
    ex = np.abs(xi - xiref).max() / np.abs(xiref).max()
    dx = np.abs(x - xo).max() / np.abs(xo).max()
    print(f"{name} inner={inner}: H {eh:.2e}  xi {ex:.2e}  cond(H) {cond:.2e}  x {dx:.2e} (bound {100 * EPS * cond:.2e})  "
          f"rn {np.abs(rn - rno).max() / max(rno):.2e}")
    assert eh <= 1e-12 and ex <= 1e-12
    assert len(rn) == inner
    assert dx <= 100 * EPS * cond
    x2 = x0.copy()
    rn2, H2, xi2 = dev.fgmres_relax(1, r0, x2, inner)
    assert x.tobytes() == x2.tobytes() and H.tobytes() == H2.tobytes() and xi.tobytes() == xi2.tobytes() and rn.tobytes() == rn2.tobytes()


def test_fgmres_relax_breaks_after_the_first_direction(mg, built):
    p, dev = _kernel_case(mg, "awkward5000")
    A, d = p.As[0], p.relaxPrecs[0]
    r0 = 1e-9 * complex_rhs(A.shape[0], 31)
    x0 = np.zeros(A.shape[0], dtype=np.complex128)                # (the update is ~1e-10: it would drown in an x of O(1))
    xo, rno = korc.FGMRES_relaxation(lambda v: A @ v, r0, x0.copy(), 3, lambda v: d * v, 1e-5)
    assert len(rno) == 1 and rno[0] < 1e-5 / 4
    x = x0.copy()
    rn, H, xi = dev.fgmres_relax(1, r0, x, 3)
    assert len(rn) == 1                                           # used = 1
    assert abs(rn[0] - rno[0]) <= 1e-10 * rno[0]               # (rn ~ ||r0||: no cancellation in t'Ht - 2 t'xi + ||r0||^2)
    assert np.abs(x - xo).max() <= 1e-11 * np.abs(xo).max()
    assert H[2, 2].real > 0                                       # the directions behind the break were summed all the same


# ---- cycles against the oracle --------------------------------------------------------------------------------------------------------
PROBLEMS = {"3lev": ([16, 16, 16], 0.5, 3), "4lev": ([16, 16, 16], 0.25, 4)}
SCHEDULES = [("Jac-GMRES", "V", 2, 2), ("Jac-GMRES", "K", 2, 1), ("Jac", "K", 2, 1), ("SPAI", "K", 2, 1), ("Jac-GMRES", "K", 1, 1)]
CYCLE_CASES = [(prob, s, False) for prob in ("3lev", "4lev") for s in SCHEDULES] + [("3lev", ("Jac-GMRES", "W", 3, 3), False),
                                                                                     ("4lev", ("Jac-GMRES", "K", 2, 1), True)]


def _param(mg, prob, sched, maxIter=5, tol=1e-10, damping=0.5):
    cells, kh, levels = PROBLEMS[prob]
    A, mesh = helmholtz(mg, cells, kh, damping)
    relax, cyc, pre, post = sched
    p = mg.getMGparam(np.complex128, np.int64, levels, 8, maxIter, tol, relax, 0.8, pre, post, cyc, "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(A, mesh, p)
    return p


_cycle_ref = {}


def _two_cycles(mg, prob, sched, scale):
    """(param, b, x after one oracle cycle, x after a second from the first iterate, trace): computed once, shared, never modified."""
    key = (prob, sched, scale)
    if key not in _cycle_ref:
        p = _param(mg, prob, sched)
        b = scale * complex_rhs(p.As[0].shape[0], 9)
        trace = []
        x1 = korc.recursiveCycle(p, b, np.zeros_like(b), 1, trace=trace).copy()
        x2 = korc.recursiveCycle(p, b, x1.copy(), 1, trace=trace).copy()
        _cycle_ref[key] = (p, b, x1, x2, trace)
    return _cycle_ref[key]


def _device_two_cycles(mg, p, b, sparse):
    dev = mg.device.DeviceHierarchy(p)
    try:
        if sparse:                                                # the coarsest solve from the complex sparse factors
            dev._set_coarse(p, force_sparse=True)
            assert dev.lib.mg_finalize(dev.handle) == 0
        x = np.zeros_like(b)
        dev.cycle(b, x, 1)
        x1 = x.copy()
        dev.cycle(b, x, -1)
        return x1, x
    finally:
        dev.close()


@pytest.mark.parametrize("prob,sched,sparse", CYCLE_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_two_cycles_against_oracle(mg, built, prob, sched, sparse):
    p, b, xo1, xo2, trace = _two_cycles(mg, prob, sched, 1.0)
    assert len(trace) > 0 and korc.rn_clear_of_tol(trace, 4.0), korc.all_rn(trace)      # on the oracle alone: the input's property
    x1, x2 = _device_two_cycles(mg, p, b, sparse)
    e1, e2 = np.abs(x1 - xo1).max() / np.abs(xo1).max(), np.abs(x2 - xo2).max() / np.abs(xo2).max()
    print(f"{prob} {sched}: cycle 1 {e1:.2e}, cycle 2 {e2:.2e}")
    assert e1 <= 1e-11 and e2 <= 1e-11


@pytest.mark.parametrize("prob,sched,sparse", CYCLE_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_two_cycles_with_the_break(mg, built, prob, sched, sparse):
    """b scaled by 1e-9: the oracle breaks after the first direction in every relaxation with inner > 1."""
    p, b, xo1, xo2, trace = _two_cycles(mg, prob, sched, 1e-9)
    assert len(trace) > 0 and korc.rn_clear_of_tol(trace, 4.0)
    assert all(rec[3] == 1 for rec in trace) and korc.all_rn(trace).max() < 1e-5 / 200
    x1, x2 = _device_two_cycles(mg, p, b, sparse)
    e1, e2 = np.abs(x1 - xo1).max() / np.abs(xo1).max(), np.abs(x2 - xo2).max() / np.abs(xo2).max()
    print(f"{prob} {sched} (break): cycle 1 {e1:.2e}, cycle 2 {e2:.2e}")
    assert e1 <= 1e-11 and e2 <= 1e-11


# ---- solveMG ----------------------------------------------------------------------------------------------------------------------------
def _solve_case(mg, p):
    """Five iterations from x = 0.  b is scaled by 1e5 so that every rn of the five cycles stays two decades or more above the
    break's 1e-5 on the oracle (asserted below; at 1e4 the four-level K(2,1) case comes down to 5.4e-4, a factor 54)."""
    b = 1e5 * complex_rhs(p.As[0].shape[0], 9)
    trace, hist = [], {}
    xo, ito = korc.solveMG(p, b, np.zeros_like(b), hist, trace)
    rn = korc.all_rn(trace)
    assert rn.size > 0 and rn.min() >= 100 * 1e-5, rn.min()         # two decades or more above the break, on the oracle alone
    x = np.zeros_like(b)
    _, _, it = mg.solveMG(p, b, x)
    dr = np.abs(p.resvec - hist["resvec"]).max() / hist["resvec"][0]
    print(f"solveMG: {it} ({ito}) iterations, resvec diff {dr:.2e}, relres {hist['resvec'][-1] / hist['resvec'][0]:.2e}")
    assert it == ito == 5 and len(p.resvec) == len(hist["resvec"])
    assert dr <= 1e-10
    assert np.abs(x - xo).max() <= 1e-10 * np.abs(xo).max()
    mg.clear_(p)


@pytest.mark.parametrize("prob", ["3lev", "4lev"])
def test_solveMG_kcycle_jac_gmres(mg, built, prob):
    _solve_case(mg, _param(mg, prob, ("Jac-GMRES", "K", 2, 1)))


def test_solveMG_with_no_pre_smoothing_on_one_level(mg, built):
    """relaxPre = 0 on level 2: FGMRES_relaxation with no columns leaves x unchanged (FGMRES.jl:119-123)."""
    p = _param(mg, "3lev", ("Jac-GMRES", "V", 2, 2))
    p.relaxPre = lambda l: 0 if l == 2 else 2
    _solve_case(mg, p)


# ---- the Krylov drivers with a K(2,1) Jac-GMRES hierarchy as preconditioner ----------------------------------------------------------------
def _oracle_prec(p, trace):
    mem = korc._Mem(p)

    def M(v):
        z = np.zeros(v.shape[0], dtype=np.complex128)
        return korc.recursiveCycle(p, np.asarray(v, dtype=np.complex128), z, 1, mem, None, trace).copy()

    return M


def _check_run(tag, got, ref, As, b):
    """tests/test_complex_krylov_gpu.py's _check_run."""
    x, flag, it, rv = got
    xo, fo, ito, rvo = ref
    dr = np.abs(rv - rvo[: len(rv)]).max() / rvo[0] if len(rv) else 0.0
    dx = np.abs(x - xo).max() / np.abs(xo).max()
    res = np.linalg.norm(b - As @ x) / np.linalg.norm(b)
    print(f"  {tag}: flag {flag} ({fo}), count {it} ({ito}), resvec diff {dr:.2e}, x diff {dx:.2e}, true residual {res:.3e}")
    assert (flag, it, len(rv)) == (fo, ito, len(rvo))
    assert dr <= 1e-8 and dx <= 1e-8
    assert res < 1e-8


def test_krylov_drivers_with_kcycle_preconditioner(mg, built):
    """The hierarchy on the damped operator (damping 0.5), the drivers on the less damped system operator (0.05).  b is scaled by
    1e6: BiCGSTAB hands the cycle its shrinking residuals, and with |b| ~ 1 their rn cross 1e-5 on the way to 1e-8."""
    cells, kh, _ = PROBLEMS["4lev"]
    As, _ = helmholtz(mg, cells, kh, 0.05)
    p = _param(mg, "4lev", ("Jac-GMRES", "K", 2, 1), maxIter=ck.MAXIT_BICGSTAB, tol=ck.TOL)
    b = 1e6 * complex_rhs(As.shape[0], 21)
    Afun = lambda v: As @ v
    trace = []
    ref = ck.bicgstb(Afun, b, ck.TOL, ck.MAXIT_BICGSTAB, _oracle_prec(p, trace))
    assert ref[1] == 0 and korc.rn_clear_of_tol(trace, 4.0), korc.all_rn(trace).min()
    x = np.zeros_like(b)
    _, _, it, nprec = mg.solveBiCGSTAB_MG_CFP64(As, p, b, x)
    _check_run("BiCGSTAB", (x, p.flag, it, p.resvec), ref, As, b)
    trace = []
    ref = ck.fgmres(Afun, b, 5, ck.TOL, ck.MAXIT_FGMRES, _oracle_prec(p, trace))
    assert ref[1] == 0 and korc.rn_clear_of_tol(trace, 4.0), korc.all_rn(trace).min()
    p.maxOuterIter = ck.MAXIT_FGMRES
    x = np.zeros_like(b)
    _, _, it, rv = mg.solveGMRES_MG_CFP64(As, p, b, x, True, 5)
    _check_run("FGMRES(5)", (x, p.flag, it, rv), ref, As, b)
    mg.clear_(p)


# ---- replaceMatrixInHierarchy on a resident K(2,1) SPAI hierarchy -------------------------------------------------------------------
def test_replace_matrix_keeps_the_device_path(mg, built):
    p = _param(mg, "4lev", ("SPAI", "K", 2, 1))
    b = complex_rhs(p.As[0].shape[0], 9)
    x = np.zeros_like(b)
    mg.recursiveCycle(p, b, x)                                    # uploads
    dev = p.device
    assert dev is not None
    cells, kh, _ = PROBLEMS["4lev"]
    A2, _ = helmholtz(mg, cells, kh, 0.3)
    mg.replaceMatrixInHierarchy(p, A2)
    assert p.device is dev                                        # refreshed in HBM, not uploaded again
    fresh = _param(mg, "4lev", ("SPAI", "K", 2, 1), damping=0.3)
    trace = []
    xo = korc.recursiveCycle(fresh, b, np.zeros_like(b), 1, trace=trace)
    assert korc.rn_clear_of_tol(trace, 4.0), korc.all_rn(trace)
    x = np.zeros_like(b)
    mg.recursiveCycle(p, b, x)
    err = np.abs(x - xo).max() / np.abs(xo).max()
    print(f"cycle after replaceMatrixInHierarchy: {err:.2e}")
    assert err <= 1e-11
    mg.clear_(p)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(mg, built):
    lib = mg.device.load_library()
    pv = _param(mg, "3lev", ("Jac", "V", 2, 1))
    b = complex_rhs(pv.As[0].shape[0], 9)
    n = b.shape[0]

    def v_cycle():
        d = mg.device.DeviceHierarchy(pv)
        try:
            x = np.zeros_like(b)
            d.cycle(b, x, 1)
            return x
        finally:
            d.close()

    x_before = v_cycle()
    p, _, xo1, _, trace = _two_cycles(mg, "3lev", ("Jac-GMRES", "K", 2, 1), 1.0)
    assert korc.rn_clear_of_tol(trace, 4.0)
    dev = mg.device.DeviceHierarchy(p)
    A8, mesh8 = mg.poisson_shifted([8, 8, 8])
    pr = mg.getMGparam(np.float64, np.int64, 2, 8, 4, 1e-10, "Jac", 0.8, 1, 1, "V")
    mg.MGsetup(A8, mesh8, pr)
    rdev = mg.device.DeviceHierarchy(pr)
    h32 = C.c_void_p()
    assert lib.mg_create_CF32(2, 1, 0, C.byref(h32)) == 0
    try:
        hc = dev.handle

        def refused(rc, code):
            assert rc == code, (rc, lib.mg_last_error())
            assert lib.mg_last_error()

        # the shared setters still refuse; the new one sorts its callers
        refused(lib.mg_set_cycle_type(hc, ord("K")), MG_ERR_UNSUPPORTED)
        refused(lib.mg_set_relax_type(hc, 1), MG_ERR_UNSUPPORTED)
        refused(lib.mg_set_schedule_CF64(h32, ord("K"), 1), MG_ERR_UNSUPPORTED)
        refused(lib.mg_set_schedule_CF64(rdev.handle, ord("K"), 1), MG_ERR_STATE)
        refused(lib.mg_set_schedule_CF64(hc, ord("Q"), 1), MG_ERR_INVALID)
        refused(lib.mg_set_schedule_CF64(hc, ord("K"), 2), MG_ERR_INVALID)
        # blocks on a K handle
        B = np.zeros((n, 2), dtype=np.complex128, order="F")
        X = np.zeros((n, 2), dtype=np.complex128, order="F")
        lz = C.c_longlong(0)
        lp = C.byref(lz)
        res = np.zeros(64)
        ab = np.array([1.0, 0.0])
        refused(lib.mg_block_cycle_CF64(hc, dz(B), dz(X), n, 2, 1), MG_ERR_UNSUPPORTED)
        refused(lib.mg_block_solve_CF64(hc, dz(B), dz(X), n, 2, 1e-6, 2, lp, dz(res)), MG_ERR_UNSUPPORTED)
        refused(lib.mg_block_spmv_CF64(hc, 1, 0, dz(ab), dz(B), dz(ab), dz(X), 2), MG_ERR_UNSUPPORTED)
        refused(lib.mg_block_bicgstab_CFP64(hc, dz(B), dz(X), n, 2, 1e-6, 2, lp, lp, dz(res), lp), MG_ERR_UNSUPPORTED)
        with pytest.raises(NotImplementedError):
            dev.block_cycle(B, X, 1)
        # mg_fgmres_relax_CF64
        r0 = complex_rhs(n, 3)
        xr = np.zeros(n, dtype=np.complex128)
        H = np.zeros(2 * 81)
        relax = lambda level, inner: lib.mg_fgmres_relax_CF64(hc, level, dz(r0), dz(xr), n, inner, 1e-5, dz(H), dz(H), dz(H), lp)
        refused(relax(1, 0), MG_ERR_INVALID)
        refused(relax(1, 9), MG_ERR_INVALID)
        refused(relax(0, 2), MG_ERR_INVALID)
        refused(relax(3, 2), MG_ERR_INVALID)                      # the coarsest level is solved, not relaxed
        refused(relax(4, 2), MG_ERR_INVALID)
        assert not xr.any()
        # relaxPre = 9 with Jac-GMRES fails at mg_finalize; a non-finalized handle is refused
        d1 = np.ascontiguousarray(p.relaxPrecs[0], dtype=np.complex128)
        assert lib.mg_set_relax_CF64(hc, 1, dz(d1), n, 9, 1) == 0
        refused(lib.mg_finalize(hc), MG_ERR_UNSUPPORTED)
        refused(relax(1, 2), MG_ERR_STATE)
        assert lib.mg_set_relax_CF64(hc, 1, dz(d1), n, 2, 1) == 0
        assert lib.mg_finalize(hc) == 0
        # the handle still runs one K cycle equal to the oracle
        x = np.zeros_like(b)
        dev.cycle(_two_cycles(mg, "3lev", ("Jac-GMRES", "K", 2, 1), 1.0)[1], x, 1)
        assert np.abs(x - xo1).max() <= 1e-11 * np.abs(xo1).max()
    finally:
        dev.close()
        rdev.close()
        lib.mg_destroy(h32)
    # the Python layer: a block of two columns against such a param
    p2 = _param(mg, "3lev", ("Jac-GMRES", "K", 2, 1))
    with pytest.raises(NotImplementedError):
        mg.solveMG(p2, np.zeros((n, 2), dtype=np.complex128, order="F"), np.zeros((n, 2), dtype=np.complex128, order="F"))
    mg.clear_(p2)
    # a V-cycle Jac handle created afterwards is bit-equal to the one created before
    assert v_cycle().tobytes() == x_before.tobytes()


def test_sync_schedule_switches_a_resident_hierarchy(mg, built):
    """cycleType / relaxType changed on the param after the upload reach the device (mg_set_schedule_CF64 through sync_schedule)."""
    p, b, xo1, _, trace = _two_cycles(mg, "3lev", ("Jac-GMRES", "K", 2, 1), 1.0)
    q = _param(mg, "3lev", ("Jac", "V", 2, 1))
    x = np.zeros_like(b)
    mg.recursiveCycle(q, b, x)                                    # resident as V(2,1) Jac
    q.cycleType, q.relaxType = "K", "Jac-GMRES"
    x = np.zeros_like(b)
    mg.recursiveCycle(q, b, x)
    assert np.abs(x - xo1).max() <= 1e-11 * np.abs(xo1).max()
    mg.clear_(q)
