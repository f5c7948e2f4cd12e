"""-m gpu: the coarsest solve by a solver object on the MI355X - param.LU a DomainDecompositionParam (one Schwarz sweep,
mg_set_coarse_dd) or a parallelJuliaSolver (its sparse factors), Float64 and ComplexF64 - the from-zero sweep
(mg_dd0_apply_*) and the chip-wide sparse coarsest factors of a CF64 hierarchy, against the existing restatements
(oracle/mg_oracle.py, tests/complex_oracle.py, tests/complex_krylov_oracle.py) given an adapter as ``LU``
(tests/coarse_solver_cases.py; the adapters are checked against a dense two-grid cycle in tests/test_coarse_solver_host.py).

Tolerances are the project's own: one cycle within 1e-12 relative max-norm, solveMG's resvec within 1e-10 * resvec[0] with
equal iteration counts, the Krylov drivers at the tolerance of tests/test_complex_krylov_gpu.py (1e-8)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import complex_krylov_oracle as ckorc
import complex_oracle as corc
import coarse_solver_cases as cs
import dd_cases
from complex_cases import complex_rhs, helmholtz
from oracle import mg_oracle as orc

pytestmark = pytest.mark.gpu

MG_ERR_INVALID, MG_ERR_STATE, MG_ERR_UNSUPPORTED = 1, 3, 4
TOL = 1e-12


def _close(x, ref, tol=TOL, what=""):
    err = cs.relmax(x, ref)
    print(f"{what} relative max-norm difference {err:.3e}")
    return err <= tol


# ---- the from-zero sweep ------------------------------------------------------------------------------------------------------
def _sweep_case(mg, name):
    if name == "2d":
        A, mesh, b, R = dd_cases.reference_case(mg)
        return A, mesh, b, [32, 32], [8, 8], [1, 1], R
    if name in ("3d", "3d-large-members"):
        n, boxes, ov = [16, 16, 8], [4, 4, 2], [1, 1, 1]
        A, mesh, b = dd_cases.poisson(mg, n, seed=2)
    elif name == "uneven":
        n, boxes, ov = [34, 30], [4, 4], [1, 1]
        A, mesh, b = dd_cases.poisson(mg, n, seed=3)
    elif name == "sequential":
        n, boxes, ov = [32, 32], [8, 8], [2, 2]
        A, mesh, b = dd_cases.poisson(mg, n, seed=4)
    else:
        n, boxes, ov = [32, 32], [8, 8], [1, 1]
        A, mesh = helmholtz(mg, n, 0.5, 0.5)
        b = complex_rhs(A.shape[0])
    return A, mesh, b, n, boxes, ov, dd_cases.Restated(mg, A, n, boxes, ov)


@pytest.mark.parametrize("name,doTranspose", [("2d", 0), ("3d", 0), ("uneven", 0), ("sequential", 0), ("complex", 0), ("complex", 1),
                                              ("3d-large-members", 0)])
def test_from_zero_sweep(mg, built, monkeypatch, name, doTranspose):
    """mg_dd0_apply* with x pre-filled with NaN equals mg_dd_apply* from zeros, and is the restatement's sweep."""
    if name == "3d-large-members":
        monkeypatch.setenv("MG_LU_MULTI_MIN_ROWS", "64")          # every member on an applier of its own, colours in sequence
    A, mesh, b, n, boxes, ov, R = _sweep_case(mg, name)
    VAL = np.complex128 if A.dtype.kind == "c" else np.float64
    p = dd_cases.dd_param(mg, A, mesh, boxes, ov, VAL=VAL)
    info = mg.DomainDecomposition.ddInfo(p, A)
    if name == "sequential":
        assert info["batched"] == 0                              # the gather form
    elif name == "3d-large-members":
        assert info["batched"] == 0 and info["launches_per_sweep"] > 3 * 32
    else:
        assert info["sequential"] == 0
    lib = mg.device.load_library()
    h = mg.DomainDecomposition._device_handle(p, A)
    sfx = "CFP64" if VAL is np.complex128 else "FP64"
    f64 = mg.device._f64
    N = A.shape[0]
    x0 = np.full(N, np.nan, dtype=VAL)
    assert getattr(lib, "mg_dd0_apply_" + sfx)(h, f64(b), f64(x0), N, doTranspose) == 0, lib.mg_last_error()
    x1 = np.zeros(N, dtype=VAL)
    assert getattr(lib, "mg_dd_apply_" + sfx)(h, f64(b), f64(x1), N, 1, doTranspose) == 0
    assert np.array_equal(x0, x1)
    assert _close(x0, R.sweep(b, np.zeros(N, dtype=VAL), 1, doTranspose), what=name)
    # the same validation as mg_dd_apply*
    assert getattr(lib, "mg_dd0_apply_" + sfx)(h, f64(b), f64(x0), N + 1, doTranspose) == MG_ERR_INVALID
    other = "FP64" if sfx == "CFP64" else "CFP64"
    z = np.zeros(2 * N)
    assert getattr(lib, "mg_dd0_apply_" + other)(h, f64(z), f64(z.copy()), N, doTranspose) == MG_ERR_STATE
    p.close()


def test_from_zero_sweep_device_pointers(mg, built):
    import torch
    A, mesh, b, R = dd_cases.reference_case(mg)
    p = dd_cases.dd_param(mg, A, mesh, [8, 8], [1, 1])
    lib = mg.device.load_library()
    h = mg.DomainDecomposition._device_handle(p, A)
    n = A.shape[0]
    buf = torch.full((n + 24,), float("nan"), dtype=torch.float64, device="cuda")
    x = buf[12:12 + n]
    bd = torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    assert lib.mg_dd0_apply_dev_FP64(h, bd.data_ptr(), x.data_ptr(), n, 0) == 0, lib.mg_last_error()
    torch.cuda.synchronize()
    assert _close(x.cpu().numpy(), R.sweep(b, np.zeros_like(b)))
    assert bool(torch.isnan(buf[:12]).all()) and bool(torch.isnan(buf[12 + n:]).all())       # nothing outside x was written
    p.close()


# ---- cycles with a Schwarz coarsest solve ------------------------------------------------------------------------------------
def _cx_case(mg, name, cyc):
    if name == "2d":
        A, mesh = helmholtz(mg, [32, 32], 0.5, 0.5)
        levels, boxes, ov, sizes = 3, [2, 2], [1, 1], [1089, 289, 81]
    else:
        A, mesh = helmholtz(mg, [16, 16, 8], 0.5, 0.5)
        levels, boxes, ov, sizes = 2, [2, 2, 2], [1, 1, 1], [2601, 405]
    p = cs.setup(mg, A, mesh, levels, cs.dd_lu(mg, mesh, boxes, ov, np.complex128), np.complex128, "Jac", 0.8, 2, 2, cyc, 12, 1e-8)
    assert [M.shape[0] for M in p.As] == sizes
    return p, cs.oracle_param(p, cs.SweepLU(mg, p, boxes, ov)), complex_rhs(A.shape[0], 9)


def _real_case(mg, name, cyc):
    if name == "3d":
        A, mesh = mg.poisson_shifted([16, 16, 8])
        levels, boxes, ov, sizes = 3, [2, 2, 1], [1, 1, 1], [2601, 405, 75]
    else:
        A, mesh = mg.poisson_shifted([32, 32])
        levels, boxes, ov, sizes = 2, [4, 4], [1, 1], [1089, 289]
    p = cs.setup(mg, A, mesh, levels, cs.dd_lu(mg, mesh, boxes, ov), np.float64, "Jac", 0.8, 2, 2, cyc, 12, 1e-8)
    assert [M.shape[0] for M in p.As] == sizes
    return p, cs.oracle_param(p, cs.SweepLU(mg, p, boxes, ov)), np.random.default_rng(9).standard_normal(A.shape[0])


def _cycles_match(mg, p, q, b, cx):
    """One cycle from x = 0 and one from a random x: twice on one handle (identical bits) and once with no_graph, each within
    1e-12 of the restatement; the coarsest solve is the Schwarz sweep."""
    cycle = corc.recursiveCycle if cx else orc.recursiveCycle
    rng = np.random.default_rng(17)
    xr = rng.standard_normal(b.size) + (1j * rng.standard_normal(b.size) if cx else 0.0)
    for x_init in (np.zeros_like(b), xr.astype(b.dtype)):
        ref = cycle(q, b, x_init.copy(), 1)
        runs = []
        for options in (None, {"no_graph": 1}):
            dev = mg.device.DeviceHierarchy(p, options=options)
            try:
                assert dev.coarse_form()["kind"] == 4 and dev.coarse_form()["order"] == p.As[-1].shape[0]
                for _ in range(2 if options is None else 1):
                    x = x_init.copy()
                    dev.cycle(b, x, -1)
                    assert _close(x, ref, what=f"cycle {p.cycleType} options={options}")
                    runs.append(x)
            finally:
                dev.close()
        assert np.array_equal(runs[0], runs[1])


@pytest.mark.parametrize("name,cyc", [("2d", "V"), ("3d", "W"), ("2d", "F")])
def test_complex_cycle_with_schwarz_coarsest(mg, built, name, cyc):
    p, q, b = _cx_case(mg, name, cyc)
    _cycles_match(mg, p, q, b, True)
    mg.clear_(p)


def test_complex_solve_mg_with_schwarz_coarsest(mg, built):
    p, q, b = _cx_case(mg, "2d", "V")
    x = np.zeros_like(b)
    _, _, iters = mg.solveMG(p, b, x)
    hist = {}
    xo, it_o = corc.solveMG(q, b, np.zeros_like(b), hist)
    ref = hist["resvec"]
    print(f"iterations {iters} / {it_o}; relative residuals {p.resvec[-1] / p.resvec[0]:.3e} / {ref[-1] / ref[0]:.3e}; "
          f"resvec difference {np.abs(p.resvec - ref).max() / ref[0]:.3e}")
    assert iters == it_o and len(p.resvec) == len(ref)
    assert np.abs(p.resvec - ref).max() <= 1e-10 * ref[0]
    assert p.resvec[-1] / p.resvec[0] < 1e-5
    assert _close(x, xo, 1e-10, "solveMG x")
    M = mg.getMultigridPreconditioner(p, b)                       # the same device hierarchy, one cycle from zero
    assert _close(M(b).copy(), corc.recursiveCycle(q, b, np.zeros_like(b), 1), what="getMultigridPreconditioner")
    mg.clear_(p)


@pytest.mark.parametrize("method", ["bicgstab", "fgmres"])
def test_complex_krylov_with_schwarz_coarsest(mg, built, method):
    p, q, b = _cx_case(mg, "2d", "V")
    A = p.As[0]
    p.maxOuterIter = 40 if method == "bicgstab" else 20
    x = np.zeros_like(b)
    Mo = ckorc.preconditioner(q)
    if method == "bicgstab":
        mg.solveBiCGSTAB_MG_CFP64(A, p, b, x)
        xo, flag, count, resvec = ckorc.bicgstb(lambda v: A @ v, b, 1e-8, 40, Mo, None)
    else:
        mg.solveGMRES_MG_CFP64(A, p, b, x, True, 10)
        xo, flag, count, resvec = ckorc.fgmres(lambda v: A @ v, b, 10, 1e-8, 20, Mo, None)
    dr = np.abs(p.resvec - resvec[:len(p.resvec)]).max() / resvec[0] if len(p.resvec) == len(resvec) else np.inf
    print(f"{method}: flag {p.flag} / {flag}, resvec lengths {len(p.resvec)} / {len(resvec)}, resvec difference {dr:.3e}")
    assert p.flag == flag and len(p.resvec) == len(resvec)
    assert dr <= 1e-8 and cs.relmax(x, xo) <= 1e-8
    mg.clear_(p)


@pytest.mark.parametrize("name,cyc", [("3d", "V"), ("3d", "W"), ("3d", "F"), ("3d", "K"), ("2d", "V")])
def test_real_cycle_with_schwarz_coarsest(mg, built, name, cyc):
    """Parity only: with one sweep as coarsest solve the restatement itself reaches relative residual 4e-3 (3-D, V) and
    2.4e-2 (2-D) in 12 cycles."""
    p, q, b = _real_case(mg, name, cyc)
    _cycles_match(mg, p, q, b, False)
    x = np.zeros_like(b)
    _, _, iters = mg.solveMG(p, b, x)
    hist = {}
    _, _, it_o = orc.solveMG(q, b, np.zeros_like(b), False, hist)
    print(f"{name} {cyc}: iterations {iters} / {it_o}, relative residual {p.resvec[-1] / p.resvec[0]:.3e}")
    assert iters == it_o and np.abs(p.resvec - hist["resvec"]).max() <= 1e-10 * hist["resvec"][0]
    mg.clear_(p)


def test_real_krylov_and_mgsolver_with_schwarz_coarsest(mg, built):
    """The single-GPU Krylov drivers and the MGsolver wrapper reach the same hierarchy."""
    p, q, b = _real_case(mg, "2d", "V")
    A = p.As[0]
    p.maxOuterIter, p.relativeTol = 30, 1e-8
    q.maxOuterIter, q.relativeTol = 30, 1e-8
    x = np.zeros_like(b)
    _, _, it, _ = mg.solveBiCGSTAB_MG(A, p, b, x)
    xo, flag, it_o, resvec = orc.solveBiCGSTAB_MG(q, b, np.zeros_like(b))
    print(f"BiCGSTAB: iterations {it} / {it_o}, flag {p.flag} / {flag}")
    assert (p.flag, it, len(p.resvec)) == (flag, it_o, len(resvec))
    assert np.abs(p.resvec - resvec).max() <= 1e-8 * resvec[0] and cs.relmax(x, xo) <= 1e-8
    xg = np.zeros_like(b)
    _, _, itg, _ = mg.solveGMRES_MG(A, p, b, xg, True, 10)
    xo, flag, it_o, resvec = orc.solveGMRES_MG(q, b, np.zeros_like(b), 10)
    print(f"FGMRES(10): inner steps {itg} / {it_o}, flag {p.flag} / {flag}")
    assert (p.flag, itg, len(p.resvec)) == (flag, it_o, len(resvec))
    assert np.abs(p.resvec - resvec).max() <= 1e-8 * resvec[0] and cs.relmax(xg, xo) <= 1e-8
    s = mg.getMGsolver(mg.copySolver(p), p.Meshes[0], 1, "BiCGSTAB")
    assert isinstance(s.MG.LU, mg.DomainDecompositionParam) and s.MG.LU is not p.LU
    X = np.zeros_like(b)
    X, s = mg.solveLinearSystem_(A, b, X, s)[:2]
    assert np.linalg.norm(b - A @ np.asarray(X).reshape(-1)) <= 1e-5 * np.linalg.norm(b)
    assert len(s.MG.LU.PrecParams) == 16                          # the copy was set up by the wrapper's own MGsetup
    mg.clear_(s.MG)
    mg.clear_(p)


# ---- a parallelJuliaSolver as coarsest solver ---------------------------------------------------------------------------------
@pytest.mark.parametrize("VAL", [np.float64, np.complex128])
def test_parallel_julia_solver_coarsest(mg, built, VAL):
    cx = VAL is np.complex128
    A, mesh = helmholtz(mg, [32, 32], 0.5, 0.5) if cx else mg.poisson_shifted([16, 16, 8])
    b = complex_rhs(A.shape[0], 9) if cx else np.random.default_rng(9).standard_normal(A.shape[0])
    p = cs.setup(mg, A, mesh, 3, cs.pjs_lu(mg, VAL), VAL, "Jac", 0.8, 2, 2, "V")
    plain = cs.setup(mg, A, mesh, 3, None, VAL, "Jac", 0.8, 2, 2, "V")
    q = cs.oracle_param(p, cs.SpluLU(p))
    x = np.zeros_like(b)
    mg.recursiveCycle(p, b, x)
    assert p.device.coarse_form() == dict(kind=1, order=p.As[-1].shape[0], launches=1)
    xd = np.zeros_like(b)
    mg.recursiveCycle(plain, b, xd)
    assert plain.device.coarse_form()["kind"] == 0
    assert _close(x, xd, what="against the default-LU hierarchy")
    cycle = corc.recursiveCycle if cx else orc.recursiveCycle
    assert _close(x, cycle(q, b, np.zeros_like(b), 1), what="against the restatement")
    if not cx:                                                    # a block of right-hand sides is served
        B = np.asfortranarray(np.random.default_rng(10).standard_normal((A.shape[0], 3)))
        X, Xd = np.zeros_like(B, order="F"), np.zeros_like(B, order="F")
        mg.recursiveCycle(p, B, X)
        mg.recursiveCycle(plain, B, Xd)
        assert p.device.coarse_form()["kind"] == 1
        assert _close(X, Xd, what="nrhs = 3")
        assert _close(X, orc.recursiveCycle(q, B, np.zeros_like(B), 1), what="nrhs = 3 against the restatement")
    mg.clear_(p)
    mg.clear_(plain)


# ---- CF64: chip-wide sparse coarsest factors ----------------------------------------------------------------------------------
@pytest.mark.parametrize("min_rows,kind", [("0", 2), ("1000000000", 1)])
def test_complex_chip_wide_coarsest(mg, built, monkeypatch, min_rows, kind):
    monkeypatch.setenv("MG_LU_MULTI_MIN_ROWS", min_rows)
    A, mesh = helmholtz(mg, [32, 32], 0.5, 0.5)
    p = cs.setup(mg, A, mesh, 2, None, np.complex128, "Jac", 0.8, 2, 2, "V")
    assert p.As[-1].shape[0] == 289
    b = complex_rhs(A.shape[0], 9)
    dev = mg.device.DeviceHierarchy(p)
    try:
        dev._set_coarse(p, force_sparse=True)
        assert dev.lib.mg_finalize(dev.handle) == 0
        form = dev.coarse_form()
        print(form)
        assert form["kind"] == kind and form["order"] == 289 and (form["launches"] > 1) == (kind == 2)
        rng = np.random.default_rng(3)
        for x_init in (np.zeros_like(b), rng.standard_normal(b.size) + 1j * rng.standard_normal(b.size)):
            ref = corc.recursiveCycle(p, b, x_init.copy(), 1)
            for _ in range(2):
                x = x_init.copy()
                dev.cycle(b, x, -1)
                assert _close(x, ref, what=f"kind {kind}")
    finally:
        dev.close()


# ---- one level ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("VAL", [np.float64, np.complex128])
def test_one_level_sweeps_from_the_callers_x(mg, built, VAL):
    cx = VAL is np.complex128
    A, mesh = helmholtz(mg, [16, 16], 0.5, 0.5) if cx else mg.poisson_shifted([16, 16])
    boxes, ov = [4, 4], [1, 1]
    p = cs.setup(mg, A, mesh, 1, cs.dd_lu(mg, mesh, boxes, ov, VAL), VAL)
    assert len(p.As) == 1
    R = dd_cases.Restated(mg, p.As[0], [16, 16], boxes, ov)
    b = complex_rhs(A.shape[0], 9) if cx else np.random.default_rng(9).standard_normal(A.shape[0])
    x0 = complex_rhs(A.shape[0], 8) if cx else np.random.default_rng(8).standard_normal(A.shape[0])
    x = x0.copy()
    mg.recursiveCycle(p, b, x)
    assert _close(x, R.sweep(b, x0.copy()), what="from the caller's x")
    x = np.zeros_like(b)
    mg.recursiveCycle(p, b, x)
    assert _close(x, R.sweep(b, np.zeros_like(b)), what="from zero")
    mg.clear_(p)


# ---- refusals and lifetime ---------------------------------------------------------------------------------------------------
def test_refusals_and_lifetime(mg, built):
    p, q, b = _real_case(mg, "3d", "V")
    lib = mg.device.load_library()
    dev = mg.device.DeviceHierarchy(p)
    h, dd = dev.handle, p.LU._handle
    try:
        ref = orc.recursiveCycle(q, b, np.zeros_like(b), 1)
        # nrhs, sharding, the device transpose
        assert lib.mg_set_nrhs(h, 2) == MG_ERR_UNSUPPORTED
        assert lib.mg_ghost_attach(h, 0, 1, 1, None) == MG_ERR_UNSUPPORTED
        assert lib.mg_transpose_hierarchy(h) == MG_ERR_UNSUPPORTED
        # an attached handle cannot be destroyed; both objects stay usable
        assert lib.mg_dd_destroy(dd) == MG_ERR_STATE
        x = np.zeros_like(b)
        dev.cycle(b, x, -1)
        assert _close(x, ref, what="cycle after the refused destroy")
        Ac = p.As[-1]
        bc = np.random.default_rng(5).standard_normal(Ac.shape[0])
        xc = np.zeros_like(bc)
        mg.solveDDSerial(Ac, bc, xc, p.LU, 1, 0)                    # stand-alone, on the attached handle
        assert p.LU._handle.value == dd.value
        assert _close(xc, q.LU.R.sweep(bc, np.zeros_like(bc)), what="stand-alone sweep on the attached handle")
        x = np.zeros_like(b)
        dev.cycle(b, x, -1)
        assert _close(x, ref, what="cycle after the stand-alone sweep")
        # the wrong value type
        Ah, mesh_h = helmholtz(mg, [8, 8], 0.5, 0.5)
        pc = dd_cases.dd_param(mg, Ah, mesh_h, [2, 2], [1, 1], VAL=np.complex128)
        assert lib.mg_set_coarse_dd(h, mg.DomainDecomposition._device_handle(pc, Ah)) == MG_ERR_STATE
        x = np.zeros_like(b)
        dev.cycle(b, x, -1)
        assert _close(x, ref, what="cycle after the refused attach")
        pc.close()
        # a handle of the wrong order: refused by mg_finalize
        A0, mesh0 = p.As[0], p.Meshes[0]
        pw = dd_cases.dd_param(mg, A0, mesh0, [2, 2, 1], [1, 1, 1])
        hw = mg.DomainDecomposition._device_handle(pw, A0)
        assert lib.mg_set_coarse_dd(h, hw) == 0
        assert lib.mg_finalize(h) == MG_ERR_INVALID
        assert lib.mg_dd_destroy(dd) == 0                         # (the first handle was detached by the second attach)
        p.LU._handle = None
        # detached: the coarsest solve is unset
        assert lib.mg_set_coarse_dd(h, None) == 0
        assert lib.mg_finalize(h) == MG_ERR_STATE and b"coarsest solve was not set" in lib.mg_last_error()
        assert lib.mg_dd_destroy(hw) == 0
        pw._handle = None
    finally:
        dev._coarse_dd = None
        dev.close()
    mg.clear_(p)


def test_python_refusals_and_transpose(mg, built):
    p, q, b = _real_case(mg, "2d", "V")
    B = np.asfortranarray(np.random.default_rng(2).standard_normal((b.size, 3)))
    with pytest.raises(NotImplementedError):
        mg.recursiveCycle(p, B, np.zeros_like(B, order="F"))
    x = np.zeros_like(b)
    mg.recursiveCycle(p, b, x)                                    # one right-hand side is served again
    assert _close(x, orc.recursiveCycle(q, b, np.zeros_like(b), 1), what="after the refused block")
    LU = p.LU
    LU.close()                                                    # close() of an attached param detaches first
    assert LU._handle is None
    mg.transposeHierarchy(p)
    assert p.LU is not LU and hasattr(p.LU, "perm_r")             # a plain factorisation (MGsetup.jl:310-311)
    x = np.zeros_like(b)
    mg.recursiveCycle(p, b, x)
    assert _close(x, orc.recursiveCycle(p, b, np.zeros_like(b), 1), what="transposed hierarchy")
    mg.clear_(p)
