"""-m gpu: the Float32 / ComplexF32 multiplicative Schwarz sweep on the MI355X (mg_dd_*_FP32 / _CFP32; opt-in
getDomainDecompositionParam(..., singleValues=True)) and a ComplexF32 hierarchy whose coarsest solve is such a sweep.

The sweep (tests/dd_single_cases.py): three evaluations of the same rounded data - E in double, the reference's own single
arithmetic, the device - with err(X) = max|X - E| / max|E| and err(device) <= YARDSTICK * err(reference) (YARDSTICK = 3,
parlu_single_cases'), after one sweep from zero and again after two more.  The two sides differ in the order and the width of their
sums only.  The shapes are the smallest ones of tests/test_dd_gpu.py, each with a path of its own: one launch per colour, 3-D, uneven
boxes, dependent colours (the sequential path), chip-wide members.

The cycle: a ComplexF32 hierarchy (shapes of test_coarse_solver_gpu._cx_case) with the single sweep as coarsest solve against the
complex128 oracle cycle on the rounded hierarchy with coarse_solver_cases.SweepLU on the rounded coarsest operator, held to what
tests/test_complex_single_gpu.py holds a ComplexF32 cycle to against that oracle: e_dev <= 4 e_ref, e_ref < 64 * 2^-24 the single
restatement's own distance."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

import coarse_solver_cases as csc
import complex_oracle as corc
import complex_single_oracle as cs32
import dd_cases
import dd_single_cases as dsc
from complex_cases import complex_rhs, helmholtz

pytestmark = pytest.mark.gpu

MG_ERR_INVALID, MG_ERR_STATE, MG_ERR_UNSUPPORTED = 1, 3, 4
C64 = np.complex64
U32 = 2.0 ** -24


def _info(mg, c, p):
    info = mg.DomainDecomposition.ddInfo(p, c.A)
    assert info["complex"] == (np.dtype(c.VAL).kind == "c") and info["single"] and info["VAL"] is c.VAL
    return info


def _held(c, x, s):
    """err(device) <= YARDSTICK * err(reference) for the iterate after s sweeps."""
    E = c.E()[s]
    e_dev, e_ref = dsc.err(x, E), dsc.err(c.reference()[s], E)
    print(f"{c.name} after {s} sweep(s): err(device) {e_dev:.3e}, err(reference) {e_ref:.3e}, bound {dsc.YARDSTICK * e_ref:.3e}")
    return e_dev <= dsc.YARDSTICK * e_ref


def _check_sweeps(mg, c, p):
    """One sweep from zero, then niter = 2 from that iterate, each held to the yardstick."""
    x = np.zeros_like(c.b)
    out, _ = mg.solveDDSerial(c.A, c.b, x, p, 1, c.t)
    assert out is x and x.dtype == np.dtype(c.VAL)
    assert _held(c, x, 1)
    mg.solveDDSerial(c.A, c.b, x, p, 2, c.t)
    assert _held(c, x, 3)


@pytest.mark.parametrize("name", ["poisson2d_f32", "helmholtz2d_c32_t0", "helmholtz2d_c32_t1"])
def test_2d_one_launch_per_colour(mg, built, name):
    c = dsc.case(mg, name)
    p = c.dd_param(mg)
    info = _info(mg, c, p)
    assert (info["numSub"], info["colours"], info["batched"], info["sequential"]) == (64, 4, 4, 0)
    assert info["launches_per_sweep"] == 4
    _check_sweeps(mg, c, p)
    p.close()


def test_3d(mg, built):
    c = dsc.case(mg, "helmholtz3d_c32_t0")
    p = c.dd_param(mg)
    info = _info(mg, c, p)
    assert (info["numSub"], info["colours"], info["batched"], info["sequential"]) == (32, 8, 8, 0)
    _check_sweeps(mg, c, p)
    p.close()


def test_uneven_boxes(mg, built):
    """34 = 4*8 + 2 and 30 = 4*7 + 2: one launch holds sub-domains of different orders and level counts."""
    c = dsc.case(mg, "uneven_f32")
    p = c.dd_param(mg)
    assert len({len(g) for g in p.GlobalIndices}) > 2
    info = _info(mg, c, p)
    assert (info["colours"], info["batched"]) == (4, 4)
    _check_sweeps(mg, c, p)
    p.close()


@pytest.mark.parametrize("name", ["dependent_f32", "dependent_c32"])
def test_dependent_colours_run_in_sequence(mg, built, name):
    """overlap 2 on cells of 4: the members run one after another - residual gather, sptrsv_lu<float> / <f2_t>, scatter-add."""
    c = dsc.case(mg, name)
    p = c.dd_param(mg)
    info = _info(mg, c, p)
    assert (info["colours"], info["batched"], info["sequential"]) == (4, 0, 4)
    assert info["launches_per_sweep"] == 3 * 64
    _check_sweeps(mg, c, p)
    p.close()


@pytest.mark.parametrize("name", ["poisson3d_f32", "helmholtz3d_c32_t1"])
def test_chip_wide_members(mg, built, monkeypatch, name):
    """MG_LU_MULTI_MIN_ROWS = 64 makes every sub-domain of the 3-D case a large member with a single applier of its own (the complex
    one swept with doTranspose = 1: the adjoint single factors)."""
    monkeypatch.setenv("MG_LU_MULTI_MIN_ROWS", "64")
    c = dsc.case(mg, name)
    p = c.dd_param(mg)
    info = _info(mg, c, p)
    assert (info["colours"], info["batched"], info["sequential"]) == (8, 0, 8)
    assert info["launches_per_sweep"] > 3 * 32
    _check_sweeps(mg, c, p)
    p.close()


def test_device_pointer_form_and_determinism(mg, built):
    """An offset view into a guarded complex64 buffer: nothing outside x is written, b is unchanged; two runs give the same bits,
    and they are the host form's."""
    import torch
    c = dsc.case(mg, "helmholtz2d_c32_t0")
    p = c.dd_param(mg)
    n = c.A.shape[0]
    guard = 7.0 - 3.0j
    bd = torch.from_numpy(c.b).cuda()
    runs = []
    for _ in range(2):
        buf = torch.full((n + 24,), guard, dtype=torch.complex64, device="cuda")
        x = buf[11:11 + n]
        x.zero_()
        out, _ = mg.solveDDSerial(c.A, bd, x, p, 1, 0)
        assert out is x
        torch.cuda.synchronize()
        assert bool((buf[:11] == guard).all()) and bool((buf[11 + n:] == guard).all())
        runs.append(x.cpu().numpy())
    assert np.array_equal(bd.cpu().numpy(), c.b)
    assert np.array_equal(runs[0], runs[1])
    assert _held(c, runs[0], 1)
    xh = np.zeros_like(c.b)
    mg.solveDDSerial(c.A, c.b, xh, p, 1, 0)
    assert np.array_equal(xh, runs[0])
    with pytest.raises(TypeError):                                       # tensors of another dtype are refused
        mg.solveDDSerial(c.A, bd.to(torch.complex128), torch.zeros(n, dtype=torch.complex128, device="cuda"), p)
    p.close()


def test_mixed_closure_in_gmres(mg, built):
    """getDDpreconditioner with a complex64 param and a complex128 B preconditions a ComplexF64 gmres: it converges to 1e-6 in at
    most one step more than with the ComplexF64 sweep on the same problem (rounding perturbs the preconditioner by about 1e-7)."""
    c = dsc.case(mg, "helmholtz2d_c32_t0")
    A, b = c.Aw.tocsr(), c.b.astype(np.complex128)
    p32 = c.dd_param(mg)
    p64 = dd_cases.dd_param(mg, A, c.mesh, c.boxes, c.overlap, VAL=np.complex128)
    M32 = mg.getDDpreconditioner(c.A, p32, b)
    assert M32(b).dtype == np.complex128
    x32, its32 = dd_cases.gmres_count(A, b, M32, rtol=1e-6)
    x64, its64 = dd_cases.gmres_count(A, b, mg.getDDpreconditioner(A, p64, b), rtol=1e-6)
    r32, r64 = (np.linalg.norm(b - A @ x) / np.linalg.norm(b) for x in (x32, x64))
    print(f"gmres steps: single sweep {its32} (relres {r32:.2e}), double sweep {its64} (relres {r64:.2e})")
    assert r32 <= 1e-6 and r64 <= 1e-6
    assert 0 < its32 <= its64 + 1
    p32.close()
    p64.close()


# ---- a ComplexF32 hierarchy with the single sweep as coarsest solve -----------------------------------------------------------
def _dd_lu32(mg, mesh, boxes, overlap):
    Ainv = mg.ParallelJuliaSolver.getParallelJuliaSolver(C64, np.int64, singleFactors=True)
    return mg.getDomainDecompositionParam(C64, np.int64, mesh, boxes, overlap, mg.getNodalIndicesOfCell, Ainv, singleValues=True)


def _cf32_case(mg, name, cyc, maxIter=12, tol=1e-8):
    """The shapes of test_coarse_solver_gpu._cx_case: (A, mesh, single param set up, boxes, overlap)."""
    if name == "2d":
        A, mesh = helmholtz(mg, [32, 32], 0.5, 0.5)
        levels, boxes, ov, sizes = 3, [2, 2], [1, 1], [1089, 289, 81]
    else:
        A, mesh = helmholtz(mg, [16, 16, 8], 0.5, 0.5)
        levels, boxes, ov, sizes = 2, [2, 2, 2], [1, 1, 1], [2601, 405]
    p = mg.getMGparam(np.complex128, np.int64, levels, 8, maxIter, tol, "Jac", 0.8, 2, 2, cyc, "NoMUMPS", 0.5, 0.0, singlePrecision=True)
    p.LU = _dd_lu32(mg, mesh, boxes, ov)
    mg.MGsetup(A, mesh, p)
    assert [M.shape[0] for M in p.As] == sizes and p.As[-1].dtype == C64
    return A, mesh, p, boxes, ov


@pytest.mark.parametrize("name,cyc", [("2d", "V"), ("2d", "W"), ("3d", "V"), ("3d", "W")])
def test_cf32_cycle_with_schwarz_coarsest(mg, built, name, cyc):
    A, mesh, p, boxes, ov = _cf32_case(mg, name, cyc)
    pr = cs32.rounded(p)
    sweep = csc.SweepLU(mg, SimpleNamespace(As=pr.As, Meshes=p.Meshes), boxes, ov)   # on the rounded coarsest operator, in double
    q = csc.oracle_param(pr, sweep)                     # the complex128 oracle cycle on the rounded hierarchy
    qs = csc.oracle_param(p, sweep)                     # the single restatement of the cycle (its coarsest solve converts back)
    b = complex_rhs(A.shape[0], 9).astype(C64)
    rng = np.random.default_rng(17)
    xr = (rng.standard_normal(b.size) + 1j * rng.standard_normal(b.size)).astype(C64)
    dev = mg.device.DeviceHierarchy(p)
    try:
        assert isinstance(dev, mg.device.ComplexSingleDeviceHierarchy)
        form = dev.coarse_form()
        assert form["kind"] == 4 and form["order"] == p.As[-1].shape[0] and form["launches"] == 2 ** len(boxes)
        assert mg.DomainDecomposition.ddInfo(p.LU, p.As[-1])["VAL"] is C64
        for x_init in (np.zeros_like(b), xr):
            xo = corc.recursiveCycle(q, b.astype(np.complex128), x_init.astype(np.complex128), 1)
            xs = cs32.recursiveCycle(qs, b, x_init.copy(), 1)
            runs = []
            for _ in range(2):
                x = x_init.copy()
                dev.cycle(b, x, -1)
                runs.append(x)
            assert np.array_equal(runs[0], runs[1])
            e_ref, e_dev = cs32.rel2(xs, xo), cs32.rel2(runs[0], xo)
            print(f"  {name} {cyc} from {'zero' if not x_init.any() else 'random x'}: restatement {e_ref:.3e}, device {e_dev:.3e} "
                  "from the double cycle")
            assert e_ref < 64 * U32
            assert e_dev <= 4 * e_ref
        with pytest.raises(NotImplementedError):        # blocks stay refused
            dev.set_nrhs(2)
        assert dev.lib.mg_set_nrhs(dev.handle, 2) == MG_ERR_UNSUPPORTED
    finally:
        dev.close()
        mg.clear_(p)


def test_cf32_public_routes_with_schwarz_coarsest(mg, built):
    """recursiveCycle, solveMG, getMultigridPreconditioner (complex64 and the mixed closure) and solveGMRES_MG_CFP64 run unchanged on
    the served param; FGMRES to 1e-8 needs at most one more inner step than the ComplexF64 hierarchy with the ComplexF64 sweep."""
    A, mesh, p, boxes, ov = _cf32_case(mg, "2d", "V", maxIter=30)
    pd = csc.setup(mg, A, mesh, 3, csc.dd_lu(mg, mesh, boxes, ov, np.complex128), np.complex128, "Jac", 0.8, 2, 2, "V", 30, 1e-8)
    b = complex_rhs(A.shape[0], 9)
    b32 = b.astype(C64)
    try:
        x1 = mg.recursiveCycle(p, b32, np.zeros_like(b32), 1)
        assert x1.dtype == C64 and p.device.coarse_form()["kind"] == 4
        z32 = mg.getMultigridPreconditioner(p, b32)(b32).copy()
        assert z32.dtype == C64 and np.array_equal(z32, x1)
        z = mg.getMultigridPreconditioner(p, b)(b)
        assert z.dtype == np.complex128 and np.array_equal(z, z32.astype(np.complex128))
        xm = np.zeros_like(b32)
        p.relativeTol = 1e-4
        _, _, it = mg.solveMG(p, b32, xm)
        assert xm.dtype == C64 and p.resvec[-1] / p.resvec[0] < 1e-4 and it < 30
        p.relativeTol = 1e-8
        xs, xd = np.zeros_like(b), np.zeros_like(b)
        mg.solveGMRES_MG_CFP64(A, p, b, xs, True, 10)
        steps_s, flag_s = len(p.resvec), p.flag
        mg.solveGMRES_MG_CFP64(A, pd, b, xd, True, 10)
        steps_d, flag_d = len(pd.resvec), pd.flag
        rs, rd = (np.linalg.norm(b - A @ x) / np.linalg.norm(b) for x in (xs, xd))
        print(f"FGMRES(10) to 1e-8: single hierarchy + single sweep {steps_s} steps (relres {rs:.2e}), double + double {steps_d} ({rd:.2e})")
        assert flag_s == 0 and flag_d == 0 and rs <= 1e-8 and rd <= 1e-8
        assert steps_s <= steps_d + 1
        LU = p.LU
        mg.replaceMatrixInHierarchy(p, A)                               # the host path: the sweep is set up again on the new coarsest matrix
        assert p.LU is LU and not mg.DomainDecomposition.isempty(LU)
        x2 = np.zeros_like(b32)
        mg.solveMG(p, b32, x2)
        assert p.device.coarse_form()["kind"] == 4
    finally:
        mg.clear_(p)
        mg.clear_(pd)
    assert mg.DomainDecomposition.isempty(p.LU) and p.LU._handle is None


def test_refusals_on_the_device(mg, built):
    """Wrong-kind entry points: MG_ERR_STATE, the handle stays usable.  Pairings of mg_set_coarse_dd: only ComplexF32 on CF32."""
    lib = mg.device.load_library()
    DD = mg.DomainDecomposition
    f32, f64 = mg.device._f32, mg.device._f64
    c, r = dsc.case(mg, "helmholtz2d_c32_t0"), dsc.case(mg, "poisson2d_f32")
    pc, pr = c.dd_param(mg), r.dd_param(mg)
    pz = dd_cases.dd_param(mg, c.Aw.tocsr(), c.mesh, c.boxes, c.overlap, VAL=np.complex128)
    n = c.A.shape[0]
    hc, hr, hz = DD._device_handle(pc, c.A), DD._device_handle(pr, r.A), DD._device_handle(pz, c.Aw.tocsr())
    zf, zd = np.zeros(2 * n, dtype=np.float32), np.zeros(2 * n)

    def state(rc, names):
        assert rc == MG_ERR_STATE, (rc, lib.mg_last_error())
        assert any(s in lib.mg_last_error() for s in names), lib.mg_last_error()

    try:
        state(lib.mg_dd_apply_FP32(hc, f32(zf), f32(zf.copy()), n, 1, 0), [b"CFP32"])
        state(lib.mg_dd0_apply_FP32(hc, f32(zf), f32(zf.copy()), n, 0), [b"CFP32"])
        state(lib.mg_dd_apply_CFP64(hc, f64(zd), f64(zd.copy()), n, 1, 0), [b"CFP32"])
        state(lib.mg_dd_apply_FP64(hc, f64(zd), f64(zd.copy()), n, 1, 0), [b"CFP32"])
        state(lib.mg_dd_apply_CFP32(hr, f32(zf), f32(zf.copy()), n, 1, 0), [b"FP32"])
        state(lib.mg_dd_apply_dev_CFP32(hr, None, None, n, 1, 0), [b"FP32"])
        state(lib.mg_dd_apply_CFP32(hz, f32(zf), f32(zf.copy()), n, 1, 0), [b"CFP64"])
        state(lib.mg_dd0_apply_dev_FP32(hz, None, None, n, 0), [b"CFP64"])
        s = pc.PrecParams[0].Ainv
        a64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
        Lp, Lc, Up, Uc = a64(s.L.indptr) + 1, a64(s.L.indices) + 1, a64(s.U.indptr) + 1, a64(s.U.indices) + 1
        i64 = mg.device._i64
        Lv, Uv = np.ascontiguousarray(s.L.data), np.ascontiguousarray(s.U.data)
        state(lib.mg_dd_set_factor_CFP32_INT64(hz, 1, s.L.shape[0], i64(Lp), i64(Lc), f32(Lv), i64(Up), i64(Uc), f32(Uv), i64(a64(s.p)),
                                               i64(a64(s.q))), [b"mg_dd_set_factor_CFP64_INT64"])
        state(lib.mg_dd_set_factor_CFP32_INT64(hr, 1, s.L.shape[0], i64(Lp), i64(Lc), f32(Lv), i64(Up), i64(Uc), f32(Uv), i64(a64(s.p)),
                                               i64(a64(s.q))), [b"mg_dd_set_factor_FP32_UINT32"])
        x = np.zeros_like(c.b)                                           # the refused calls left the handles usable
        mg.solveDDSerial(c.A, c.b, x, pc, 1, 0)
        assert _held(c, x, 1)
        # mg_set_coarse_dd: a CF32, a CF64 and an FP64 hierarchy against sweeps of each kind
        Ah, mesh = helmholtz(mg, [8, 8], 0.5, 0.5)
        ps = mg.getMGparam(np.complex128, np.int64, 2, 8, 8, 1e-6, "Jac", 0.8, 1, 1, "V", "NoMUMPS", 0.5, 0.0, singlePrecision=True)
        pd = mg.getMGparam(np.complex128, np.int64, 2, 8, 8, 1e-6, "Jac", 0.8, 1, 1, "V", "NoMUMPS", 0.5, 0.0)
        mg.MGsetup(Ah, mesh, ps)
        mg.MGsetup(Ah, mesh, pd)
        sdev, ddev = mg.device.DeviceHierarchy(ps), mg.device.DeviceHierarchy(pd)
        try:
            for h, other in ((sdev.handle, hr), (ddev.handle, hc), (ddev.handle, hr)):
                state(lib.mg_set_coarse_dd(h, other), [b"Float32", b"ComplexF32"])
            assert lib.mg_set_coarse_dd(sdev.handle, hz) == MG_ERR_UNSUPPORTED            # a ComplexF64 sweep on a CF32 handle: as before
            assert b"not served for CF32 handles" in lib.mg_last_error()
            # a ComplexF32 sweep is accepted by the CF32 hierarchy; its order must then be the coarsest level's (mg_finalize)
            assert lib.mg_set_coarse_dd(sdev.handle, hc) == 0, lib.mg_last_error()
            assert lib.mg_finalize(sdev.handle) == MG_ERR_INVALID
            assert lib.mg_dd_destroy(hc) == MG_ERR_STATE                                  # borrowed
            assert lib.mg_set_coarse_dd(sdev.handle, None) == 0
        finally:
            sdev.close()
            ddev.close()
            mg.clear_(ps)
            mg.clear_(pd)
    finally:
        for p in (pc, pr, pz):
            DD.clear_(p)
