"""-m gpu: the GMRES coarsest solve of complex hierarchies on the MI355X (mg_set_coarse_gmres_CF64, mg_coarse_gmres_CF64, the CGDOT
epilogue of cx_csr_stream_spmv, the chain passes and the one-workgroup tail of csrc/mg_cxvec.hpp) against the oracles of
tests/complex_coarse_cases.py on the same host-built hierarchies.

Tolerances come from the project's own complex tests.  On the CPU, relative noise of 1e-13 on every A z of the coarsest solve moved x
after two cycles by 0.2 to 1.3 x 1e-13 and x of the stand-alone solves by at most 2.9 x 1e-13: 1e-11 keeps a margin of about 30 over
n * eps-sized errors.  Estimates: 1e-10 relative.  The two device paths (chain of passes / one-workgroup tail) differ in the order of
their sums only: 1e-12.  solveMG: resvec within 1e-10 * resvec[0].  ComplexF32: 64 * U32 in the rel2 measure of
tests/test_complex_block_gpu.py.  The break at err <= 0.01 is a discrete decision: every comparison first asserts ON THE ORACLE'S LOG
ALONE a clearance of 1.5 (complex_coarse_cases.clearance)."""
import copy
import ctypes as C

import numpy as np
import pytest

import complex_coarse_cases as cc
import complex_kcycle_oracle as korc
import complex_krylov_oracle as ck
import complex_oracle as corc
import complex_single_oracle as cs
from complex_cases import complex_rhs

pytestmark = pytest.mark.gpu

MG_ERR_INVALID, MG_ERR_STATE, MG_ERR_UNSUPPORTED = 1, 3, 4
U32 = 2.0 ** -24
_dp = C.POINTER(C.c_double)
dz = lambda a: a.ctypes.data_as(_dp)
CHAIN, TAIL = 0.0, -1.0           # values of the option coarse_gmres_tail_rows: the chain everywhere / the default threshold


def _set_path(dev, value):
    assert dev.lib.mg_set_option(dev.handle, b"coarse_gmres_tail_rows", float(value)) == 0


def _dense_reference_cycle(mg):
    """One V(2,1) Jac cycle on a dense-inverse handle of its own: the existing path, bit for bit."""
    p = cc.hierarchy(mg, "3lev", coarse="NoMUMPS")
    b = cc.cycle_rhs(p)
    dev = mg.device.DeviceHierarchy(p)
    try:
        assert dev.coarse_form()["kind"] == 0
        x = np.zeros_like(b)
        dev.cycle(b, x, 1)
        dev.cycle(b, x, -1)
        return x
    finally:
        dev.close()


@pytest.fixture(scope="module")
def dense_before(mg, built):
    return _dense_reference_cycle(mg)


# ---- the solve alone, row by row ------------------------------------------------------------------------------------------------------
_solve_devs = {}


def _solve_dev(mg, name):
    if name not in _solve_devs:
        p = cc.manual_param(mg, cc.solve_case(name)[0])
        _solve_devs[name] = (p, mg.device.DeviceHierarchy(p))
    return _solve_devs[name]


@pytest.fixture(scope="module", autouse=True)
def _close_solve_devs(dense_before):
    yield
    for _, dev in _solve_devs.values():
        dev.close()
    _solve_devs.clear()


@pytest.mark.parametrize("name", cc.SOLVE_CASES)
def test_solve_alone_against_oracle(mg, built, name):
    A, d, b, orc, xo = cc.solve_case(name)
    flag_o, steps_o, res_o = orc.log[0]
    assert cc.clearance(orc.log) >= cc.MIN_CLEARANCE
    assert (steps_o, flag_o == 0) == cc.solve_expected(name)
    n = A.shape[0]
    if name.startswith("awkward"):
        assert A.indptr[2001] - A.indptr[2000] >= 3000 and d[2000] != 0 and b[2000] != 0      # the long row feeds every partial
        assert n % 256 != 0 and n > 1024
    p, dev = _solve_dev(mg, name)
    form = dev.coarse_form()
    assert form["kind"] == 3 and form["order"] == n
    got = {}
    for path, launches in ((CHAIN, 2 + sum(i + 3 for i in range(10)) + 1), (TAIL, 1 + 2 * 10 + 1)):
        _set_path(dev, path)
        assert dev.coarse_form()["launches"] == launches          # the budget: at most i + 3 launches in step i; 2 with the tail
        x, flag, res = dev.coarse_gmres(b)
        ex = np.abs(x - xo).max() / np.abs(xo).max()
        er = np.abs(res - res_o[:len(res)]).max() / np.abs(res_o).max() if len(res) == steps_o else np.inf
        print(f"{name} {'chain' if path == CHAIN else 'tail'}: steps {len(res)} (oracle {steps_o}) flag {flag} ({flag_o})  x {ex:.2e}  "
              f"estimates {er:.2e}  clearance {cc.clearance(orc.log):.2f}")
        assert len(res) == steps_o and flag == flag_o
        assert np.abs(res - res_o).max() <= 1e-10 * np.abs(res_o).max()
        assert ex <= 1e-11
        x2, flag2, res2 = dev.coarse_gmres(b)                      # a rerun adds the same numbers in the same order
        assert x.tobytes() == x2.tobytes() and res.tobytes() == res2.tobytes() and flag2 == flag
        got[path] = x
    e = np.abs(got[CHAIN] - got[TAIL]).max() / np.abs(xo).max()
    print(f"{name}: chain against tail {e:.2e}")
    assert e <= 1e-12


def test_solve_alone_zero_right_hand_side(mg, built):
    p, dev = _solve_dev(mg, "awkward5000_f0.3")
    n = p.As[-1].shape[0]
    for path in (CHAIN, TAIL):
        _set_path(dev, path)
        x, flag, res = dev.coarse_gmres(np.zeros(n, dtype=np.complex128))
        assert flag == -9 and len(res) == 0 and not np.isnan(x).any() and not x.any()
    _set_path(dev, TAIL)


# ---- cycles against the oracle --------------------------------------------------------------------------------------------------------
_cycle_ref = {}


def _oracle_two_cycles(mg, name):
    """(param, b, x1, x2, the oracle's log): computed once, shared, never modified."""
    if name not in _cycle_ref:
        p = cc.hierarchy(mg, name)
        q = cc.oracle_param(p)
        b = cc.cycle_rhs(p)
        cyc = korc.recursiveCycle if name == "3levK" else corc.recursiveCycle
        x1 = cyc(q, b, np.zeros_like(b), 1).copy()
        x2 = cyc(q, b, x1.copy(), 1).copy()
        _cycle_ref[name] = (p, b, x1, x2, q.LU.log)
    return _cycle_ref[name]


@pytest.mark.parametrize("name,wide", [("2lev", 0), ("3lev", 0), ("4lev", 0), ("3levK", 0), ("3lev", 1)])
def test_two_cycles_against_oracle(mg, built, name, wide):
    p, b, x1o, x2o, log = _oracle_two_cycles(mg, name)
    assert cc.clearance(log) >= cc.MIN_CLEARANCE
    dev = mg.device.DeviceHierarchy(p, options={"force_rowptr64": wide})
    try:
        assert dev.coarse_form()["kind"] == 3
        x = np.zeros_like(b)
        dev.cycle(b, x, 1)
        e1 = np.abs(x - x1o).max() / np.abs(x1o).max()
        dev.cycle(b, x, -1)
        e2 = np.abs(x - x2o).max() / np.abs(x2o).max()
        print(f"{name} wide={wide}: coarsest rows {p.As[-1].shape[0]}, oracle solves {[(f, s) for f, s, _ in log]}, clearance "
              f"{cc.clearance(log):.2f}; x1 {e1:.2e} x2 {e2:.2e}")
        assert e1 <= 1e-11 and e2 <= 1e-11
    finally:
        dev.close()


def test_single_level_hierarchy_is_the_solve_alone(mg, built):
    A, d, b, orc, xo = cc.solve_case("S100_f1.5")
    p = mg.getMGparam(np.complex128, np.int64, 1, 8, 4, 1e-10, "Jac", 0.8, 1, 1, "V", "GMRES")
    p.As, p.Ps, p.Rs, p.relaxPrecs = [A], [], [], []
    p.LU = np.ascontiguousarray(d, dtype=np.complex128)
    p.nrhs = 1
    dev = mg.device.DeviceHierarchy(p)
    try:
        x = complex_rhs(A.shape[0], 77)                                # x is set to zero first (MGcycle.jl:153)
        dev.cycle(b, x, 0)
        assert np.abs(x - xo).max() <= 1e-11 * np.abs(xo).max()
    finally:
        dev.close()


def test_solveMG_against_oracle(mg, built):
    p = cc.hierarchy(mg, "2lev", maxIter=8)
    q = cc.oracle_param(p)
    b = cc.cycle_rhs(p)
    hist = {}
    xo, ito = corc.solveMG(q, b, np.zeros_like(b), hist)
    assert cc.clearance(q.LU.log) >= cc.MIN_CLEARANCE
    try:
        x = np.zeros_like(b)
        _, _, it = mg.solveMG(p, b, x)
        e = np.abs(p.resvec - hist["resvec"]).max() / hist["resvec"][0]
        print(f"solveMG 2lev: {it} cycles (oracle {ito}), clearance {cc.clearance(q.LU.log):.2f}, resvec {e:.2e}, final relres {p.resvec[-1] / p.resvec[0]:.2e}")
        assert it == ito and len(p.resvec) == len(hist["resvec"])
        assert e <= 1e-10
    finally:
        mg.clear_(p)


# ---- the drivers and the wrapper ------------------------------------------------------------------------------------------------------
def _c1_gmres(mg):
    """Case C1 of tests/complex_krylov_oracle.py with the hierarchy's coarsest solve switched to GMRES, on a copy (the shared case is
    never modified)."""
    from multigrid_jl_amd.mgsetup import defineCoarsestAinv
    p0, As, b = ck.case(mg, "C1")
    p = copy.copy(p0)
    p.coarseSolveType = "GMRES"
    p.LU = None
    p.device = None
    defineCoarsestAinv(p, p.As[-1])
    assert isinstance(p.LU, np.ndarray)
    return p, As, b


@pytest.mark.parametrize("method", ["fgmres", "bicgstab"])
def test_drivers_converge_with_the_gmres_coarsest_solve(mg, built, method):
    p, As, b = _c1_gmres(mg)
    x = np.zeros_like(b)
    try:
        if method == "fgmres":
            p.maxOuterIter = ck.MAXIT_FGMRES
            _, _, it, _ = mg.solveGMRES_MG_CFP64(As, p, b, x, True, 10)
        else:
            p.maxOuterIter = ck.MAXIT_BICGSTAB
            _, _, it, _ = mg.solveBiCGSTAB_MG_CFP64(As, p, b, x)
        res = np.linalg.norm(b - As @ x) / np.linalg.norm(b)
        print(f"C1 {method} with the GMRES coarsest solve: {it} iterations, flag {p.flag}, true residual {res:.3e} "
              f"(LU coarsest solve: {ck.EXPECTED['C1']['bicgstab' if method == 'bicgstab' else 10]})")
        assert p.flag in (0, -3) and res <= ck.TOL
    finally:
        mg.clear_(p)


def test_wrapper_and_lifecycle(mg, built):
    """A complex MGsolver("GMRES") through solveLinearSystem_, then copySolver / getMultigridPreconditioner / destroyCoarsestLU / clear_."""
    from complex_cases import helmholtz
    A, mesh = helmholtz(mg, [16] * 3, 0.5, 0.5)
    p = mg.getMGparam(np.complex128, np.int64, 3, 8, 30, 1e-8, "Jac", 0.8, 2, 1, "V", "GMRES", 0.5, 0.0)
    s = mg.getMGsolver(p, mesh, 2, "GMRES")
    B = complex_rhs(A.shape[0], 31)
    X = np.zeros_like(B)
    try:
        mg.solveLinearSystem_(A, B, X, s)
        res = np.linalg.norm(A @ X - B) / np.linalg.norm(B)
        print(f"  MGsolver('GMRES'), coarseSolveType GMRES: {s.nIter} iterations, flag {p.flag}, ||A X - B|| / ||B|| = {res:.3e}")
        assert p.flag in (0, -3) and s.nIter > 0 and res < s.tol
        assert p.device is not None and p.device.coarse_form()["kind"] == 3
        M = mg.getMultigridPreconditioner(p, B)
        q = cc.oracle_param(p)
        zo = corc.recursiveCycle(q, B, np.zeros_like(B), 1)
        assert cc.clearance(q.LU.log) >= cc.MIN_CLEARANCE
        assert np.abs(M(B) - zo).max() <= 1e-11 * np.abs(zo).max()
        p2 = mg.copySolver(p)
        assert p2.coarseSolveType == "GMRES" and p2.LU is None and not p2.As
        mg.destroyCoarsestLU(p)
        assert p.LU is None
    finally:
        mg.clear_(p)
    assert p.device is None and p.LU is None


# ---- ComplexF32 -----------------------------------------------------------------------------------------------------------------------
def test_single_precision_cycle_against_oracle(mg, built):
    p = cc.hierarchy(mg, "3lev", single=True)
    assert p.As[-1].dtype == np.complex64 and p.LU.dtype == np.complex64
    q = cc.oracle_param(p)                                             # the coarsest solve in complex128 on widened inputs
    b = cc.cycle_rhs(p).astype(np.complex64)
    xo = cs.recursiveCycle(q, b, np.zeros_like(b), 1).copy()
    assert cc.clearance(q.LU.log) >= cc.MIN_CLEARANCE
    dev = mg.device.DeviceHierarchy(p)
    try:
        assert dev.coarse_form()["kind"] == 3
        x = np.zeros_like(b)
        dev.cycle(b, x, 1)
        e = cs.rel2(x, xo)
        print(f"ComplexF32 3lev: oracle solves {[(f, s) for f, s, _ in q.LU.log]}, clearance {cc.clearance(q.LU.log):.2f}, rel2 {e:.2e} "
              f"(bound {64 * U32:.2e})")
        assert e < 64 * U32
    finally:
        dev.close()


# ---- re-setup ---------------------------------------------------------------------------------------------------------------------------
def test_replace_matrix_stays_on_the_device(mg, built):
    from complex_cases import helmholtz
    p = cc.hierarchy(mg, "3lev")
    b = cc.cycle_rhs(p)
    try:
        mg.recursiveCycle(p, b, np.zeros_like(b), 1)
        dev = p.device
        assert dev is not None and dev.coarse_form()["kind"] == 3
        A2, mesh = helmholtz(mg, [16, 16, 16], 0.5, 0.35)              # a new medium on the same pattern
        assert np.array_equal(A2.indptr, p.As[0].indptr) and np.array_equal(A2.indices, p.As[0].indices)
        mg.replaceMatrixInHierarchy(p, A2)
        assert p.device is dev and dev.coarse_form()["kind"] == 3     # the same handle: no upload, no factorisation
        ref = 0.8 / p.As[-1].diagonal()
        assert isinstance(p.LU, np.ndarray) and np.abs(p.LU - ref).max() <= 1e-14 * np.abs(ref).max()
        fresh = mg.getMGparam(np.complex128, np.int64, 3, 8, 8, 1e-10, "Jac", 0.8, 2, 1, "V", "GMRES", 0.5, 0.0)
        mg.MGsetup(A2, mesh, fresh)
        q = cc.oracle_param(fresh)
        xo = corc.recursiveCycle(q, b, np.zeros_like(b), 1).copy()
        assert cc.clearance(q.LU.log) >= cc.MIN_CLEARANCE
        x = np.zeros_like(b)
        mg.recursiveCycle(p, b, x, 1)
        e = np.abs(x - xo).max() / np.abs(xo).max()
        print(f"re-setup 3lev: oracle solves {[(f, s) for f, s, _ in q.LU.log]}, clearance {cc.clearance(q.LU.log):.2f}, x {e:.2e}")
        assert e <= 1e-11
    finally:
        mg.clear_(p)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(mg, built):
    p, b, x1o, _, log = _oracle_two_cycles(mg, "3lev")
    assert cc.clearance(log) >= cc.MIN_CLEARANCE
    n, nc = p.As[0].shape[0], p.As[-1].shape[0]
    lib = mg.device.load_library()
    d = np.ascontiguousarray(p.LU, dtype=np.complex128)
    bc = complex_rhs(nc, 5)
    xc = np.zeros_like(bc)
    steps, flag = C.c_longlong(0), C.c_longlong(0)
    res = np.zeros(10)
    gm = lambda h, m: lib.mg_coarse_gmres_CF64(h, dz(bc), dz(xc), m, C.byref(steps), C.byref(flag), dz(res))
    # a real handle
    Ar, meshr = mg.poisson_shifted([8, 8, 8])
    pr = mg.getMGparam(np.float64, np.int64, 2, 8, 4, 1e-10, "Jac", 0.8, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(Ar, meshr, pr)
    devr = mg.device.DeviceHierarchy(pr)
    try:
        assert lib.mg_set_coarse_gmres_CF64(devr.handle, nc, dz(d)) == MG_ERR_STATE
        assert gm(devr.handle, nc) == MG_ERR_STATE
    finally:
        devr.close()
    # a dense-inverse complex handle
    pd = cc.hierarchy(mg, "3lev", coarse="NoMUMPS")
    devd = mg.device.DeviceHierarchy(pd)
    try:
        assert gm(devd.handle, nc) == MG_ERR_STATE
    finally:
        devd.close()
    dev = mg.device.DeviceHierarchy(p)
    try:
        assert gm(dev.handle, nc + 1) == MG_ERR_INVALID and gm(dev.handle, nc) == 0
        B = np.asfortranarray(np.stack([b, 2 * b], axis=1))
        X = np.zeros_like(B)
        it, fl, cnt = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        assert lib.mg_block_cycle_CF64(dev.handle, dz(B), dz(X), n, 2, 1) == MG_ERR_UNSUPPORTED
        assert lib.mg_block_bicgstab_CFP64(dev.handle, dz(B), dz(X), n, 2, 1e-8, 5, C.byref(it), C.byref(fl), dz(np.zeros(11)),
                                           C.byref(cnt)) == MG_ERR_UNSUPPORTED
        assert not X.any()
        with pytest.raises(NotImplementedError):
            dev.block_cycle(B, X, 1)
        # a Jacobi vector of the wrong order: caught at mg_finalize; until then the coarsest solve alone is refused too
        assert lib.mg_set_coarse_gmres_CF64(dev.handle, nc + 1, dz(np.ones(nc + 1, dtype=np.complex128))) == 0
        assert gm(dev.handle, nc) == MG_ERR_STATE                       # not finalized
        assert lib.mg_finalize(dev.handle) == MG_ERR_INVALID
        assert lib.mg_set_coarse_gmres_CF64(dev.handle, nc, dz(d)) == 0 and lib.mg_finalize(dev.handle) == 0
        x = np.zeros_like(b)
        dev.cycle(b, x, 1)
        e = np.abs(x - x1o).max() / np.abs(x1o).max()
        print(f"after the refusals: x {e:.2e}")
        assert e <= 1e-11
    finally:
        dev.close()
        mg.clear_(pr)


# ---- the existing paths are untouched ---------------------------------------------------------------------------------------------------
def test_dense_inverse_cycles_are_bit_equal_before_and_after(mg, built, dense_before):
    """(last in this file: a V(2,1) Jac handle with the dense inverse created before and after everything above)"""
    assert _dense_reference_cycle(mg).tobytes() == dense_before.tobytes()
