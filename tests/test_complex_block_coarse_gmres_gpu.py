"""-m gpu: the block GMRES coarsest solve of complex hierarchies on the MI355X (option coarse_gmres_blocks / blockCoarseGMRES=True;
mg_block_coarse_gmres_CF64, cx_coarse_block_gmres, the passes of csrc/mg_cxblk_coarse.hpp) against the oracles of
tests/complex_block_coarse_cases.py: the block solve alone, and whole-block cycles on host-built hierarchies.

Tolerances are the project's for the single-vector solve: steps and flag equal, estimates within 1e-10 relative,
max|X - Xo| / max|Xo| <= 1e-11, resvec of solveMG within 1e-10 * resvec[0], ComplexF32 within 64 * 2^-24 in the rel2 measure of
tests/test_complex_block_gpu.py.  On the CPU, relative noise of 1e-13 on every A_c Z_j moved the block oracle's X by at most 4.1e-13
(awkward5000_f0.3, k = 16; 1.8e-13 to 4.0e-13 on the other cases) and its estimates by at most 2.2e-14 (S100_f1.5, k = 2):
tests/test_complex_block_coarse_gmres_host.py repeats that run and holds every case to a quarter of its tolerance.  The break at
err <= 0.01 is a discrete decision: every comparison first asserts ON THE ORACLE'S LOG ALONE a clearance of 1.5.
The two device paths (chain of grid-wide passes / one-workgroup form, which a block of n_c * k <= 8192 values admits) differ in the
order of their sums only: 1e-12.  The option coarse_gmres_tail_rows picks the path: 0 the chain, 8192 the one-workgroup form wherever it
is admitted, -1 the measured default."""
import ctypes as C

import numpy as np
import pytest

import complex_block_coarse_cases as cbc
import complex_coarse_cases as cc
import complex_single_oracle as cs
from complex_cases import helmholtz

pytestmark = pytest.mark.gpu

MG_ERR_UNSUPPORTED = 4
U32 = 2.0 ** -24
_dp = C.POINTER(C.c_double)
dz = lambda a: a.ctypes.data_as(_dp)
CHAIN, TAIL, DEFAULT = 0.0, 8192.0, -1.0                  # values of the option coarse_gmres_tail_rows
LAUNCHES = {CHAIN: 3 + sum(j + 5 for j in range(10)) + 1,  # the budget: 3 for the front, at most j + 5 in step j, the combination
            TAIL: 1 + 2 * 10 + 1}                          # one launch for the front, the product and one launch per step


def _set_path(dev, value):
    assert dev.lib.mg_set_option(dev.handle, b"coarse_gmres_tail_rows", float(value)) == 0


# ---- the existing paths, before anything else in this file ------------------------------------------------------------------------------
def _dense_reference(mg):
    """One V(2,1) Jac cycle (two calls) and one 4-column block cycle on a dense-inverse handle of its own: the existing paths."""
    p = cc.hierarchy(mg, "3lev", coarse="NoMUMPS")
    b = cc.cycle_rhs(p)
    B = cbc.cycle_rhs(p, 4)
    dev = mg.device.DeviceHierarchy(p)
    try:
        assert dev.coarse_form()["kind"] == 0
        x = np.zeros_like(b)
        dev.cycle(b, x, 1)
        dev.cycle(b, x, -1)
        X = np.zeros_like(B)
        dev.block_cycle(B, X, 1)
        return x.tobytes(), X.tobytes()
    finally:
        dev.close()


@pytest.fixture(scope="module")
def dense_before(mg, built):
    return _dense_reference(mg)


# ---- the solve alone ------------------------------------------------------------------------------------------------------------------
_solve_devs = {}


def _solve_dev(mg, name):
    if name not in _solve_devs:
        p = cc.manual_param(mg, cc.solve_case(name)[0])
        p.blockCoarseGMRES = True
        _solve_devs[name] = (p, mg.device.DeviceHierarchy(p))
    return _solve_devs[name]


@pytest.fixture(scope="module", autouse=True)
def _close_solve_devs(dense_before):
    yield
    for _, dev in _solve_devs.values():
        dev.close()
    _solve_devs.clear()


def _check_solve(mg, name, k, zero):
    A, d, B, orc, Xo = cbc.solve_case(name, k, zero_column=zero)
    flag_o, steps_o, res_o = orc.log[0]
    assert cbc.clearance(orc.log) >= cbc.MIN_CLEARANCE
    n = A.shape[0]
    if name.startswith("awkward"):
        assert A.indptr[2001] - A.indptr[2000] >= 3000 and d[2000] != 0 and B[2000].all()      # the long row feeds every partial
        assert n % 256 != 0 and n > 1024
    p, dev = _solve_dev(mg, name)
    assert dev.coarse_form()["kind"] == 3
    got = {}
    try:
        for path in (CHAIN, TAIL):
            _set_path(dev, path)
            admitted = path == CHAIN or n * k <= 8192
            form = dev.block_coarse_form(k)
            assert form == dict(served=True, launches=LAUNCHES[path if admitted else CHAIN], path=int(path == TAIL and admitted))
            if not admitted:
                continue
            X, flag, res = dev.block_coarse_gmres(B)
            ex = np.abs(X - Xo).max() / np.abs(Xo).max()
            er = np.abs(res - res_o[:len(res)]).max() / np.abs(res_o).max() if len(res) == steps_o else np.inf
            print(f"{name} k={k} zero={zero} {'chain' if path == CHAIN else 'one workgroup'}: steps {len(res)} (oracle {steps_o}) flag {flag} "
                  f"({flag_o})  X {ex:.2e}  estimates {er:.2e}  clearance {cbc.clearance(orc.log):.2f}")
            assert len(res) == steps_o and flag == flag_o
            assert np.abs(res - res_o).max() <= 1e-10 * np.abs(res_o).max()
            assert ex <= 1e-11
            X2, flag2, res2 = dev.block_coarse_gmres(B)            # a rerun adds the same numbers in the same order
            assert X.tobytes() == X2.tobytes() and res.tobytes() == res2.tobytes() and flag2 == flag
            got[path] = X
    finally:
        _set_path(dev, DEFAULT)
    if name.startswith("awkward"):
        assert TAIL not in got and n * k > 8192                    # 5000 rows: the chain is the only path of a block
    else:
        e = np.abs(got[CHAIN] - got[TAIL]).max() / np.abs(Xo).max()
        print(f"{name} k={k}: chain against one workgroup {e:.2e}")
        assert e <= 1e-12
    return got[CHAIN], Xo


@pytest.mark.parametrize("name,k", sorted(cbc.SOLVE_RUNS))
def test_block_solve_alone_against_oracle(mg, built, name, k):
    assert cbc.solve_case(name, k)[3].log[0][:2] == cbc.SOLVE_RUNS[(name, k)][::-1]
    _check_solve(mg, name, k, False)


def test_block_solve_zero_column_gives_exact_zeros(mg, built):
    name, k = cbc.ZERO_COLUMN
    X, Xo = _check_solve(mg, name, k, True)
    assert not Xo[:, 1].any() and not X[:, 1].any() and not np.isnan(X).any()
    p, dev = _solve_dev(mg, name)
    assert dev.block_coarse_form(k)["path"] == 1                   # by default this level takes the one-workgroup form
    X1, _, _ = dev.block_coarse_gmres(cbc.solve_case(name, k, zero_column=True)[2])
    assert not X1[:, 1].any() and np.abs(X1 - Xo).max() <= 1e-11 * np.abs(Xo).max()


def test_block_solve_of_one_column_is_the_vector_solve(mg, built):
    A, d, b, orc, xo = cc.solve_case("S100_f1.5")
    p, dev = _solve_dev(mg, "S100_f1.5")
    x1, f1, r1 = dev.coarse_gmres(b)
    X, f, r = dev.block_coarse_gmres(b.reshape(-1, 1))
    assert X[:, 0].tobytes() == x1.tobytes() and f == f1 and r.tobytes() == r1.tobytes()


def test_block_solve_zero_right_hand_side(mg, built):
    p, dev = _solve_dev(mg, "awkward5000_f0.3")
    n = p.As[-1].shape[0]
    for k in (2, 16):
        X, flag, res = dev.block_coarse_gmres(np.zeros((n, k), dtype=np.complex128))
        assert flag == -9 and len(res) == 0 and not np.isnan(X).any() and not X.any()
    ps, devs = _solve_dev(mg, "S100_f1.5")                         # ... and the one-workgroup form
    assert devs.block_coarse_form(3)["path"] == 1
    X, flag, res = devs.block_coarse_gmres(np.zeros((100, 3), dtype=np.complex128))
    assert flag == -9 and len(res) == 0 and not np.isnan(X).any() and not X.any()
    A, d, B, orc, Xo = cbc.solve_case("awkward5000_f0.3", 2)       # the handle stays usable
    X, flag, res = dev.block_coarse_gmres(B)
    assert np.abs(X - Xo).max() <= 1e-11 * np.abs(Xo).max()


# ---- cycles against the whole-block oracle ---------------------------------------------------------------------------------------------
_cycle_ref = {}


def _oracle_two_cycles(mg, name, k):
    """(param, B, X1, X2, the oracle's log): computed once, shared, never modified."""
    if (name, k) not in _cycle_ref:
        p = cbc.hierarchy(mg, name)
        q = cbc.oracle_param(p)
        B = cbc.cycle_rhs(p, k)
        X1 = cbc.block_cycle(q, B, np.zeros_like(B))
        X2 = cbc.block_cycle(q, B, X1)
        _cycle_ref[(name, k)] = (p, B, X1, X2, q.LU.log)
    return _cycle_ref[(name, k)]


@pytest.mark.parametrize("wide", [0, 1], ids=["int", "rowptr64"])
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("name", sorted(cbc.HIERARCHIES))
def test_two_block_cycles_against_oracle(mg, built, name, k, wide):
    p, B, X1o, X2o, log = _oracle_two_cycles(mg, name, k)
    assert cbc.clearance(log) >= cbc.MIN_CLEARANCE
    dev = mg.device.DeviceHierarchy(p, options={"force_rowptr64": wide})
    try:
        assert dev.coarse_form()["kind"] == 3 and dev.block_coarse_form(k)["served"]
        for path in (CHAIN, TAIL):                                 # (every coarsest level here admits the one-workgroup form)
            _set_path(dev, path)
            assert dev.block_coarse_form(k)["path"] == int(path == TAIL)
            X = np.zeros_like(B)
            dev.block_cycle(B, X, 1)
            e1 = np.abs(X - X1o).max() / np.abs(X1o).max()
            dev.block_cycle(B, X, -1)
            e2 = np.abs(X - X2o).max() / np.abs(X2o).max()
            print(f"{name} k={k} wide={wide} {'chain' if path == CHAIN else 'one workgroup'}: coarsest rows {p.As[-1].shape[0]}, oracle "
                  f"solves {[(f, s) for f, s, _ in log]}, clearance {cbc.clearance(log):.2f}; X1 {e1:.2e} X2 {e2:.2e}")
            assert e1 <= 1e-11 and e2 <= 1e-11
    finally:
        dev.close()


def test_block_solveMG_against_oracle(mg, built):
    p = cbc.hierarchy(mg, "16_2lev", maxIter=8)
    q = cbc.oracle_param(p)
    B = cbc.cycle_rhs(p, 2)
    Xo, ito, reso = cbc.block_solveMG(q, B, np.zeros_like(B))
    assert cbc.clearance(q.LU.log) >= cbc.MIN_CLEARANCE
    try:
        X = np.zeros_like(B)
        _, _, it = mg.solveMG(p, B, X)
        e = np.abs(p.resvec - reso).max() / reso[0] if len(p.resvec) == len(reso) else np.inf
        print(f"block solveMG 16_2lev: {it} cycles (oracle {ito}), clearance {cbc.clearance(q.LU.log):.2f}, resvec {e:.2e}, "
              f"final relres {p.resvec[-1] / p.resvec[0]:.2e}")
        assert it == ito and len(p.resvec) == len(reso)
        assert e <= 1e-10
    finally:
        mg.clear_(p)


def test_single_precision_block_cycle_against_oracle(mg, built):
    p = cbc.hierarchy(mg, "16_3levV", single=True)
    assert p.As[-1].dtype == np.complex64 and p.LU.dtype == np.complex64 and p.blockCoarseGMRES
    q = cbc.oracle_param(p)                                            # the coarsest solve in complex128 on widened inputs
    B = cbc.cycle_rhs(p, 2)
    Xo = cbc.block_cycle_single(q, B)
    assert cbc.clearance(q.LU.log) >= cbc.MIN_CLEARANCE
    try:
        X = mg.getMultigridPreconditioner(p, B)(B)
        e = cs.rel2(X, Xo)
        print(f"ComplexF32 16_3levV k=2: oracle solves {[(f, s) for f, s, _ in q.LU.log]}, clearance {cbc.clearance(q.LU.log):.2f}, "
              f"rel2 {e:.2e} (bound {64 * U32:.2e})")
        assert X.dtype == np.complex128 and e < 64 * U32
    finally:
        mg.clear_(p)


def test_single_precision_handle_runs_the_block_solve_alone_in_double(mg, built):
    """mg_block_coarse_gmres_CF64 on a ComplexF32 handle: the solve runs in ComplexF64 on the widened coarsest operator, so it is held to
    the ComplexF64 tolerances against the oracle on that widened operator."""
    p = cbc.hierarchy(mg, "16_2lev", single=True)
    Ac, d = p.As[-1].astype(np.complex128), np.asarray(p.LU, dtype=np.complex128)
    B = cbc.cb.block_rhs(Ac.shape[0], 3)
    orc = cbc.OracleBlockCoarseGmres(Ac, d)
    Xo = orc.solve(B)
    flag_o, steps_o, res_o = orc.log[0]
    assert cbc.clearance(orc.log) >= cbc.MIN_CLEARANCE
    dev = mg.device.DeviceHierarchy(p)
    try:
        assert dev.coarse_form()["kind"] == 3 and dev.block_coarse_form(3)["served"]
        for path in (CHAIN, TAIL):
            _set_path(dev, path)
            X, flag, res = dev.block_coarse_gmres(B)
            ex = np.abs(X - Xo).max() / np.abs(Xo).max()
            print(f"ComplexF32 handle, {Ac.shape[0]} rows, k=3, {'chain' if path == CHAIN else 'one workgroup'}: steps {len(res)} ({steps_o}) "
                  f"flag {flag} ({flag_o}) X {ex:.2e} clearance {cbc.clearance(orc.log):.2f}")
            assert len(res) == steps_o and flag == flag_o
            assert np.abs(res - res_o).max() <= 1e-10 * np.abs(res_o).max() and ex <= 1e-11
    finally:
        dev.close()
        mg.clear_(p)


# ---- the block drivers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["bicgstab", "fgmres"])
def test_block_drivers_converge_with_the_block_gmres_coarsest_solve(mg, built, method):
    p = cbc.hierarchy(mg, "16_2lev", maxIter=60, tol=1e-8)
    A = p.As[0]
    B = cbc.cycle_rhs(p, 4)
    X = np.zeros_like(B)
    try:
        if method == "bicgstab":
            _, _, it, _ = mg.solveBlockBiCGSTAB_MG_CFP64(None, p, B, X)
            res = (np.linalg.norm(B - A @ X, axis=0) / np.linalg.norm(B, axis=0)).max()
        else:
            p.maxOuterIter = 10
            _, _, it, _ = mg.solveBlockGMRES_MG_CFP64(None, p, B, X, True, 10)
            res = np.linalg.norm(B - A @ X) / np.linalg.norm(B)
        print(f"16_2lev block {method}, 4 columns, block GMRES coarsest solve: {it} iterations, flag {p.flag}, true residual {res:.3e}")
        assert p.flag in (0, -3) and res <= 1e-8
    finally:
        mg.clear_(p)


def test_block_solver_wrapper(mg, built):
    """A complex MGsolver("BiCGSTAB") given a block; MGsolver("GMRES") given a block stays refused."""
    A, mesh = helmholtz(mg, [16] * 3, 0.5, 0.5)
    n = A.shape[0]
    B = cbc.cb.block_rhs(n, 2)
    p = mg.getMGparam(np.complex128, np.int64, 2, 8, 60, 1e-8, "Jac", 0.8, 2, 1, "V", "GMRES", 0.5, 0.0, blockCoarseGMRES=True)
    s = mg.getMGsolver(p, mesh, 2, "BiCGSTAB")
    X = np.zeros_like(B)
    try:
        mg.solveLinearSystem_(A, B, X, s)
        res = (np.linalg.norm(B - A @ X, axis=0) / np.linalg.norm(B, axis=0)).max()
        print(f"MGsolver('BiCGSTAB') on a block, block GMRES coarsest solve: {s.nIter} iterations, flag {p.flag}, residual {res:.3e}")
        assert p.flag in (0, -3) and res < s.tol and p.device.block_coarse_form(2)["served"]
        sg = mg.getMGsolver(p, mesh, 2, "GMRES")
        with pytest.raises(NotImplementedError):
            mg.solveLinearSystem_(A, B, np.zeros_like(B), sg)
    finally:
        mg.clear_(p)


# ---- re-setup and the adjoint ----------------------------------------------------------------------------------------------------------
def test_block_cycle_after_replace_matrix_and_after_adjoint(mg, built):
    p = cbc.hierarchy(mg, "16_3levV")
    B = cbc.cycle_rhs(p, 2)
    try:
        mg.recursiveCycle(p, B, np.zeros_like(B), 1)
        dev = p.device
        A2, mesh = helmholtz(mg, [16] * 3, 0.5, 0.25)                  # a new medium on the same pattern
        assert np.array_equal(A2.indptr, p.As[0].indptr) and np.array_equal(A2.indices, p.As[0].indices)
        mg.replaceMatrixInHierarchy(p, A2)
        assert p.device is dev and dev.coarse_form()["kind"] == 3 and dev.block_coarse_form(2)["served"]
        fresh = cbc.hierarchy(mg, "16_3levV", damping=0.25)
        q = cbc.oracle_param(fresh)
        Xo = cbc.block_cycle(q, B, np.zeros_like(B))
        assert cbc.clearance(q.LU.log) >= cbc.MIN_CLEARANCE
        X = np.zeros_like(B)
        mg.recursiveCycle(p, B, X, 1)
        e = np.abs(X - Xo).max() / np.abs(Xo).max()
        print(f"re-setup: oracle solves {[(f, s) for f, s, _ in q.LU.log]}, clearance {cbc.clearance(q.LU.log):.2f}, X {e:.2e}")
        assert e <= 1e-11
        mg.adjointHierarchy(p)                                         # the host mirror and the resident hierarchy, flipped
        assert p.device is dev
        qa = cbc.oracle_param(p)
        Xa = cbc.block_cycle(qa, B, np.zeros_like(B))
        assert cbc.clearance(qa.LU.log) >= cbc.MIN_CLEARANCE
        X = np.zeros_like(B)
        mg.recursiveCycle(p, B, X, 1)
        e = np.abs(X - Xa).max() / np.abs(Xa).max()
        print(f"adjoint: oracle solves {[(f, s) for f, s, _ in qa.LU.log]}, clearance {cbc.clearance(qa.LU.log):.2f}, X {e:.2e}")
        assert e <= 1e-11
        mg.clear_(fresh)
    finally:
        mg.clear_(p)


# ---- the opt-in -------------------------------------------------------------------------------------------------------------------------
def test_option_off_refuses_and_single_vector_cycles_are_bit_equal(mg, built):
    p0 = cbc.hierarchy(mg, "16_3levV", opt_in=False)
    p1 = cbc.hierarchy(mg, "16_3levV")
    n = p0.As[0].shape[0]
    b = cc.cycle_rhs(p0)
    B = cbc.cycle_rhs(p0, 2)
    lib = mg.device.load_library()
    dev0, dev1 = mg.device.DeviceHierarchy(p0), mg.device.DeviceHierarchy(p1)
    try:
        assert not dev0.block_coarse_form(2)["served"] and dev1.block_coarse_form(2)["served"]
        X = np.full(B.shape, 3.0 - 2.0j, order="F")
        keep = X.copy()
        assert lib.mg_block_cycle_CF64(dev0.handle, dz(B), dz(X), n, 2, 1) == MG_ERR_UNSUPPORTED
        assert X.tobytes() == keep.tobytes()
        nc = p0.As[-1].shape[0]
        Bc, Xc = np.asfortranarray(B[:nc]), np.zeros((nc, 2), dtype=np.complex128, order="F")
        assert lib.mg_block_coarse_gmres_CF64(dev0.handle, dz(Bc), dz(Xc), nc, 2, None, None, None) == MG_ERR_UNSUPPORTED
        assert lib.mg_block_coarse_gmres_CF64(dev1.handle, dz(Bc), dz(Xc), nc, 17, None, None, None) == MG_ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError):
            dev0.block_cycle(B, X, 1)
        x0, x1 = np.zeros_like(b), np.zeros_like(b)
        for dev, x in ((dev0, x0), (dev1, x1)):
            dev.cycle(b, x, 1)
            dev.cycle(b, x, -1)
        assert x0.tobytes() == x1.tobytes() and np.abs(x0).max() > 0
        dev1.block_cycle(B, X, 1)                                      # ... also behind a block call on the opted-in handle
        x2 = np.zeros_like(b)
        dev1.cycle(b, x2, 1)
        dev1.cycle(b, x2, -1)
        assert x2.tobytes() == x0.tobytes()
    finally:
        dev0.close()
        dev1.close()


# ---- the existing paths are untouched ---------------------------------------------------------------------------------------------------
def test_dense_inverse_cycles_are_bit_equal_before_and_after(mg, built, dense_before):
    """(last in this file: a V(2,1) Jac handle with the dense inverse, one vector and a block of 4 columns, created before and after
    everything above)"""
    assert _dense_reference(mg) == dense_before
