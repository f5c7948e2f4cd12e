"""-m gpu: the Vanka cell-block smoother inside the complex cycle (relaxation type 2 of a CF64 / CF32 handle) - recursiveCycle,
solveMG, the preconditioner closure, the _CFP64 drivers and a complex MGsolver on hierarchies built by MGsetup with
``complexVanka=True``, against the numpy restatement of tests/complex_vanka_cases.py; the from-zero mode of the relaxation against
the general path on a zero x, bit for bit; and the return codes of the C ABI.

Bounds.  ComplexF64 cycles: 1e-11 of max|x|, the bound of tests/test_complex_kcycle_gpu.py for complex cycles (the stand-alone
complex relaxation is held to 1e-12; restriction, coarsest solve and prolongation come on top).  K-cycle: max(1e-11, 10 d), d the
restatement's own distance between its plain run and a run with the Gram dots in long double - see test_kcycle.  ComplexF32 cycles:
at most 4 e_ref from the complex128 restatement on the rounded hierarchy, e_ref the complex64 restatement's distance from the same
comparand (the rule of tests/test_complex_single_gpu.py: the same expression in the same order at unit round-off 2^-24, differing
in FMA contraction and in how the complex product is formed).  The condition on the inputs - every residual factor of the
restatement below 0.5 - is tests/test_complex_vanka_host.py::test_restatement_contracts."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import complex_krylov_oracle as ck
import complex_vanka_cases as CV
import vanka_cases as V
from complex_kcycle_oracle import rn_clear_of_tol

pytestmark = pytest.mark.gpu

TOL = 1e-11
MG_ERR_INVALID, MG_ERR_STATE, MG_ERR_UNSUPPORTED = 1, 3, 4
C64 = np.complex64

# id -> (case, options of complex_vanka_cases.param)
CYCLES = {
    "32v": ("32v", {}), "32w": ("32w", {}), "24v": ("24v", {}), "24w": ("24w", {}), "12v": ("12v", {}), "16v": ("16v", {}),
    "24f": ("24v", {"cycle": "F"}),
    "24v-econ": ("24v", {"relaxType": "EconVankaFaces"}),
    "24v-add": ("24v", {"relaxType": "VankaFacesAdd"}),
    "24v-pair": ("24v", {"w": (0.7, 0.5)}),
}


@pytest.mark.parametrize("cid", list(CYCLES))
def test_recursive_cycle(mg, built, cid):
    """A first cycle from zero and a second from its result."""
    name, kw = CYCLES[cid]
    p, H, b, xs, _, _ = CV.reference(mg, name, 2, **kw)
    x = np.zeros_like(b)
    mg.recursiveCycle(p, b, x)
    e1 = CV.err_max(x, xs[0])
    mg.recursiveCycle(p, b, x)
    e2 = CV.err_max(x, xs[1])
    print(f"{cid}: first cycle {e1:.3e}, second cycle {e2:.3e} of max|x|")
    assert e1 <= TOL and e2 <= TOL


def test_schedule_follows_param(mg, built):
    """cycleType and the sweep counts changed on the param after the upload reach the resident hierarchy (blocks stay)."""
    _, _, b, xv, _, _ = CV.reference(mg, "24v", 2)
    _, _, _, xw, _, _ = CV.reference(mg, "24w", 2)
    p = CV.param(mg, "24v", maxIter=7)                      # (a param of its own: the shared ones keep their schedule)
    x = np.zeros_like(b)
    mg.recursiveCycle(p, b, x)
    assert CV.err_max(x, xv[0]) <= TOL
    dev = p.device
    p.cycleType = "W"
    x = np.zeros_like(b)
    mg.recursiveCycle(p, b, x)
    assert p.device is dev and CV.err_max(x, xw[0]) <= TOL
    p.cycleType = "V"
    p.relaxPre = lambda level: 0                            # a count of 0: no iteration (unlike the pointwise relax)
    H = CV.Hier(p)
    ref = CV.restate_cycle(H, b, None, True, "V")
    x = np.zeros_like(b)
    mg.recursiveCycle(p, b, x)
    assert p.device is dev and CV.err_max(x, ref) <= TOL


_kcase = {}


def _kcycle(mg):
    """The K case with its bound: (reference of 5 cycles, d)."""
    if not _kcase:
        ref = CV.reference(mg, "32k", 5)
        p, H, b, xs, res, trace = ref
        assert rn_clear_of_tol(trace) and all(rec[3] == 2 for rec in trace)      # the breaks are discrete decisions (none taken)
        tr = []
        xl, _ = CV.restate_history(H, b, 5, "K", fgmres=CV.FGMRES_relaxation_ld, trace=tr)
        assert [rec[3] for rec in tr] == [rec[3] for rec in trace]
        _kcase["v"] = (ref, max(CV.err_max(a, c) for a, c in zip(xl, xs)))
    return _kcase["v"]


def test_kcycle(mg, built):
    """K(1,1) on [32,32], three levels: level 2 runs two FGMRES steps preconditioned by its own cycle.  The bound comes from the
    restatement: d is the distance (of max|x|, the largest over five cycles) between its plain run and a run whose Gram dots are
    summed in long double; the device's sums run in a third order, hence max(1e-11, 10 d).  d measured on the CPU: 6.5e-15 in the first cycle, below 2e-15 in
    the others (printed below); the bound is therefore 1e-11."""
    (p, H, b, xs, _, trace), d = _kcycle(mg)
    bound = max(TOL, 10.0 * d)
    print(f"K-cycle: d = {d:.3e}, bound {bound:.3e}")
    x = np.zeros_like(b)
    mg.recursiveCycle(p, b, x)
    e1 = CV.err_max(x, xs[0])
    mg.recursiveCycle(p, b, x)
    e2 = CV.err_max(x, xs[1])
    print(f"K-cycle: first cycle {e1:.3e}, second cycle {e2:.3e} of max|x|")
    assert e1 <= bound and e2 <= bound


@pytest.mark.parametrize("name", ["32v", "32w", "32k", "12v"])
def test_solve_mg_history(mg, built, name):
    if name == "32k":
        (p, H, b, xs, res, _), d = _kcycle(mg)
        bound = max(TOL, 10.0 * d)
    else:
        p, H, b, xs, res, _ = CV.reference(mg, name, 5)
        bound = TOL
    assert p.maxOuterIter == 5 and p.relativeTol == 1e-30
    x = np.zeros_like(b)
    _, _, iters = mg.solveMG(p, b, x)
    e = np.abs(p.resvec - res).max() / res[0]
    ex = CV.err_max(x, xs[-1])
    print(f"{name}: residual history {e:.3e} of resvec[0], x {ex:.3e} (bound {bound:.1e}); factors {np.round(p.resvec[1:] / p.resvec[:-1], 3)}")
    assert iters == 5 and p.resvec.shape == res.shape
    assert np.all(np.abs(p.resvec - res) <= 1e-10 * res[0]) and ex <= bound


def _raw_cycle(dev, b, x_is_zero, single):
    x = np.zeros_like(b)
    if single:
        fp = C.POINTER(C.c_float)
        rc = dev.lib.mg_cycle_CF32(dev.handle, b.ctypes.data_as(fp), x.ctypes.data_as(fp), b.size, 1, x_is_zero)
    else:
        dp = C.POINTER(C.c_double)
        rc = dev.lib.mg_cycle_CF64(dev.handle, b.ctypes.data_as(dp), x.ctypes.data_as(dp), b.size, 1, x_is_zero)
    assert rc == 0
    return x


@pytest.mark.parametrize("single", [False, True], ids=["CF64", "CF32"])
@pytest.mark.parametrize("relaxType", ["VankaFaces", "VankaFacesAdd"])
@pytest.mark.parametrize("name", ["24v", "12v"])
def test_from_zero_mode_is_the_general_path_on_zero(mg, built, name, relaxType, single):
    """x_is_zero = 1 (the first pass of the fine level reads b and the blocks only) against x_is_zero = 0 on a zero x (the general
    pass walks the matrix): the same bits.  Two runs of the same call: the same bits."""
    p = CV.param(mg, name, single=single, relaxType=relaxType)
    b = CV.rhs(p.As[0].shape[0], single)
    mg.adjustMemoryForNumRHS(p, 1)
    dev = mg.to_device(p)
    xz = _raw_cycle(dev, b, 1, single)
    xg = _raw_cycle(dev, b, 0, single)
    xz2 = _raw_cycle(dev, b, 1, single)
    xg2 = _raw_cycle(dev, b, 0, single)
    assert xz.dtype == (C64 if single else np.complex128) and np.abs(xz).max() > 0 and np.all(np.isfinite(xz.view(xz.real.dtype)))
    assert np.array_equal(xz, xg)
    assert np.array_equal(xz, xz2) and np.array_equal(xg, xg2)
    xh = np.zeros_like(b)
    mg.recursiveCycle(p, b, xh)                     # (norm(x) decides: the from-zero call)
    assert np.array_equal(xh, xz)


@pytest.mark.parametrize("name", ["32v", "32w", "12v"])
def test_cf32_cycles(mg, built, name):
    p = CV.param(mg, name, single=True)
    Hs, Ho = CV.Hier(p), CV.Hier(p, widen=True)
    b = CV.rhs(p.As[0].shape[0], True)
    cyc = p.cycleType
    x = np.zeros_like(b)
    xs, xo = None, None
    for k in range(2):                              # from zero, then each from its own first iterate
        mg.recursiveCycle(p, b, x)
        assert x.dtype == C64
        xs = CV.restate_cycle(Hs, b, xs, k == 0, cyc)
        xo = CV.restate_cycle(Ho, b.astype(np.complex128), xo, k == 0, cyc)
        assert xs.dtype == C64 and xo.dtype == np.complex128
        e_ref, e_dev = CV.rel2(xs, xo), CV.rel2(x, xo)
        print(f"{name} CF32 cycle {k + 1}: restatement {e_ref:.3e}, device {e_dev:.3e} from the complex128 cycle on the rounded hierarchy")
        assert e_ref < 64 * 2.0 ** -24
        assert e_dev <= 4 * e_ref


def _helmholtz_K(n, omega):
    """K = A_real - omega^2 (1 - 0.01i) S with S the 0/1 face selector (A_real - A_damped) / (omega^2 (1 - 0.1i))."""
    Ar = V.mixed_operator(n, True)
    Ad = CV.operator(n, omega)
    S = ((Ar - Ad) / (omega ** 2 * (1.0 - 0.1j))).tocsr()
    S = sp.csr_matrix(np.round(S.real))
    assert set(np.unique(S.diagonal())) == {0.0, 1.0} and (S - sp.diags(S.diagonal())).nnz == 0
    K = sp.csr_matrix(Ar.astype(np.complex128) - omega ** 2 * (1.0 - 0.01j) * S)
    K.sort_indices()
    return K


def test_preconditioner_is_the_first_cycle(mg, built):
    p, H, b, xs, _, _ = CV.reference(mg, "32v", 2)
    Mfun = mg.getMultigridPreconditioner(p, b)
    assert CV.err_max(Mfun(b), xs[0]) <= TOL
    assert CV.err_max(Mfun(b), xs[0]) <= TOL        # (the closure zeroes its iterate)


@pytest.mark.parametrize("single", [False, True], ids=["CF64", "CF32"])
def test_drivers(mg, built, single):
    """FGMRES(5) and BiCGSTAB on the lightly damped K, preconditioned by one cycle of the hierarchy built on the 0.1-damped operator."""
    n, _, omega, _ = CV.CASES["32v"]
    K = _helmholtz_K(n, omega)
    p = CV.param(mg, "32v", single=single, maxIter=10, tol=1e-8)
    b = CV.rhs(K.shape[0])
    H = CV.Hier(p)
    if single:
        M = lambda v: CV.restate_cycle(H, v.astype(C64), None, True, "V").astype(np.complex128)
    else:
        M = lambda v: CV.restate_cycle(H, v, None, True, "V")
    _, flag_o, it_o, _ = ck.fgmres(lambda v: K @ v, b, 5, 1e-8, 10, M=M)
    assert flag_o == 0
    x = np.zeros_like(b)
    _, _, it, resvec = mg.solveGMRES_MG_CFP64(K, p, b, x, True, 5)
    r = np.linalg.norm(b - K @ x) / np.linalg.norm(b)
    print(f"FGMRES(5) single={single}: {it} inner steps (oracle {it_o}), true residual {r:.3e}")
    assert p.flag == 0 and abs(it - it_o) <= 1 and r <= 1e-6
    x = np.zeros_like(b)
    _, _, itb, _ = mg.solveBiCGSTAB_MG_CFP64(K, p, b, x)
    r = np.linalg.norm(b - K @ x) / np.linalg.norm(b)
    print(f"BiCGSTAB single={single}: {itb} iterations, true residual {r:.3e}")
    assert p.flag == 0 and r <= 1e-6


def test_mgsolver_gmres(mg, built):
    n, levels, omega, _ = CV.CASES["32v"]
    A = CV.operator(n, omega)
    p = mg.copySolver(CV.param(mg, "32v", maxIter=10, tol=1e-8))
    assert p.complexVanka and not mg.hierarchyExists(p)
    s = mg.getMGsolver(p, CV.mesh(mg, n), 0, "GMRES")
    b = CV.rhs(A.shape[0])
    x = np.zeros_like(b)
    mg.solveLinearSystem_(A, b, x, s)
    r = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    print(f"MGsolver GMRES: {s.nIter} inner steps, true residual {r:.3e}")
    assert mg.hierarchyExists(s.MG) and s.MG.relaxPrecs[0].dtype == C64 and 0 < s.nIter <= 50 and r <= 1e-6
    mg.clearSolver_(s)


def test_cabi_refusals(mg, built):
    lib = mg.device.load_library()
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    p, H, b, xs, _, _ = CV.reference(mg, "24v", 2)
    nn = np.ascontiguousarray(p.Meshes[0].n, dtype=np.int64)
    blk = np.asfortranarray(p.relaxPrecs[0])
    args = (1, 2, nn.ctypes.data_as(C.POINTER(C.c_longlong)), 1, 1, blk.ctypes.data_as(fp))
    # an FP64 handle; a complex level without its operator; the other precision's entry
    h = C.c_void_p()
    assert lib.mg_create(2, 1, 0, C.byref(h)) == 0
    assert lib.mg_set_vanka_CF64(h, *args) == MG_ERR_STATE and lib.mg_set_vanka_relax_CF64(h, ord("V")) == MG_ERR_STATE
    assert lib.mg_destroy(h) == 0
    h = C.c_void_p()
    assert lib.mg_create_CF64(2, 1, 0, C.byref(h)) == 0
    assert lib.mg_set_vanka_CF64(h, *args) == MG_ERR_STATE
    assert b"upload the operator" in lib.mg_last_error()
    assert lib.mg_set_vanka_CF32(h, *args) == MG_ERR_STATE and lib.mg_set_vanka_relax_CF32(h, ord("V")) == MG_ERR_STATE
    assert lib.mg_destroy(h) == 0

    def cycle_ok(dev, bb, ref, tol):
        x = np.zeros_like(bb)
        dev.cycle(bb, x, 1)
        assert CV.err_max(x, ref) <= tol

    mg.adjustMemoryForNumRHS(p, 1)
    dev = mg.to_device(p)
    hd = dev.handle
    # the setters that stay closed to type 2, geometry and type checks, then the handle still serves
    assert lib.mg_set_schedule_CF64(hd, ord("V"), 2) == MG_ERR_INVALID and lib.mg_set_relax_type(hd, 2) == MG_ERR_UNSUPPORTED
    assert lib.mg_set_vanka_relax_CF64(hd, ord("Q")) == MG_ERR_INVALID
    bad = (1, 2, nn.ctypes.data_as(C.POINTER(C.c_longlong)), 0, 1, blk.ctypes.data_as(fp))         # faces only: another row count
    assert lib.mg_set_vanka_CF64(hd, *bad) == MG_ERR_INVALID
    lex = (1, 2, nn.ctypes.data_as(C.POINTER(C.c_longlong)), 1, 4, blk.ctypes.data_as(fp))
    assert lib.mg_set_vanka_CF64(hd, *lex) == MG_ERR_UNSUPPORTED
    cycle_ok(dev, b, xs[0], TOL)
    # blocks of right-hand sides and the device re-setup
    B = np.asfortranarray(np.stack([b, b], axis=1))
    X = np.zeros_like(B, order="F")
    assert lib.mg_block_cycle_CF64(hd, B.ctypes.data_as(dp), X.ctypes.data_as(dp), b.size, 2, 1) == MG_ERR_UNSUPPORTED and not X.any()
    nz = np.ascontiguousarray(np.conj(p.As[0].data))
    om = np.full(p.levels, 0.6)
    done = C.c_longlong(0)
    assert lib.mg_rap_CF64(hd, nz.ctypes.data_as(dp), nz.size, 0, om.ctypes.data_as(dp), C.byref(done)) == MG_ERR_UNSUPPORTED
    cycle_ok(dev, b, xs[0], TOL)
    # leaving Vanka mode and coming back
    assert lib.mg_set_schedule_CF64(hd, ord("V"), 0) == 0 and lib.mg_finalize(hd) == 0
    x = np.zeros_like(b)
    dev.cycle(b, x, 1)
    assert x.any() and CV.err_max(x, xs[0]) > 1e-3                                                  # (d = 0: the coarse correction alone)
    assert lib.mg_set_vanka_relax_CF64(hd, ord("V")) == 0 and lib.mg_finalize(hd) == 0
    cycle_ok(dev, b, xs[0], TOL)
    # a level that lacks blocks: a pointwise complex hierarchy asked for type 2
    pj = mg.getMGparam(np.complex128, np.int64, 3, 1, 5, 1e-8, "Jac", 0.6, 1, 1, "V", "NoMUMPS", 0.4, 0.0, "SystemsFacesMixedLinear")
    n = CV.CASES["24v"][0]
    mg.MGsetup(CV.operator(n, 0.15), CV.mesh(mg, n), pj)
    dj = mg.to_device(pj)
    xj = np.zeros_like(b)
    dj.cycle(b, xj, 1)
    assert lib.mg_set_vanka_relax_CF64(dj.handle, ord("V")) == 0 and lib.mg_finalize(dj.handle) == MG_ERR_STATE
    assert b"has no blocks" in lib.mg_last_error()
    assert lib.mg_set_schedule_CF64(dj.handle, ord("V"), 0) == 0 and lib.mg_finalize(dj.handle) == 0
    xj2 = np.zeros_like(b)
    dj.cycle(b, xj2, 1)
    assert xj.any() and np.array_equal(xj, xj2)
    dj.close()
    pj.device = None
    # a CF32 handle with 'K'
    ps = CV.param(mg, "24v", single=True)
    mg.adjustMemoryForNumRHS(ps, 1)
    ds = mg.to_device(ps)
    b32 = CV.rhs(b.size, True)
    x32 = np.zeros_like(b32)
    ds.cycle(b32, x32, 1)
    assert lib.mg_set_vanka_CF64(ds.handle, *args) == MG_ERR_STATE
    assert lib.mg_set_vanka_relax_CF32(ds.handle, ord("K")) == 0 and lib.mg_finalize(ds.handle) == MG_ERR_UNSUPPORTED
    assert lib.mg_set_vanka_relax_CF32(ds.handle, ord("V")) == 0 and lib.mg_finalize(ds.handle) == 0
    y32 = np.zeros_like(b32)
    ds.cycle(b32, y32, 1)
    assert x32.any() and np.array_equal(x32, y32)
