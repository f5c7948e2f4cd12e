"""-m gpu: the multiplicative Schwarz sweep on the MI355X (mg_dd_*, multigrid.jl_amd/domain_decomposition.py) against its
numpy restatement (tests/dd_cases.py) on the same index lists, with scipy's splu as the sub-domain solver.

Tolerance: relative max-norm 1e-12, what one composite cycle is held to against its restatement (tests/test_complex_gpu.py) -
after one sweep from x = 0 and again after two more sweeps from that iterate.  Both sides solve well-conditioned
sub-domain systems (principal sub-matrices of at most 11^2 / 7^3 rows) with different factorisation orderings; the
device residual sums a row's 5-27 products in eight strided parts."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import dd_cases
from complex_cases import complex_rhs, helmholtz

pytestmark = pytest.mark.gpu

MG_ERR_INVALID, MG_ERR_STATE = 1, 3
TOL = 1e-12


def _close(x, ref):
    err = np.abs(x - ref).max() / np.abs(ref).max()
    print(f"relative max-norm difference {err:.3e}")
    return err <= TOL


def _check_sweeps(mg, A, b, p, R, doTranspose=0):
    """One sweep from zero, then niter = 2 from that iterate, each against the restatement."""
    x = np.zeros_like(b)
    ref = np.zeros_like(b)
    out, _ = mg.solveDDSerial(A, b, x, p, 1, doTranspose)
    assert out is x
    R.sweep(b, ref, 1, doTranspose)
    assert _close(x, ref)
    mg.solveDDSerial(A, b, x, p, 2, doTranspose)
    R.sweep(b, ref, 2, doTranspose)
    assert _close(x, ref)


def _info(mg, A, p):
    return mg.DomainDecomposition.ddInfo(p, A)


def test_reference_problem_2d(mg, built):
    A, mesh, b, R = dd_cases.reference_case(mg)
    p = dd_cases.dd_param(mg, A, mesh, [8, 8], [1, 1])
    info = _info(mg, A, p)
    assert (info["numSub"], info["colours"], info["batched"], info["sequential"]) == (64, 4, 4, 0)
    assert info["launches_per_sweep"] <= 8 and not info["complex"]
    _check_sweeps(mg, A, b, p, R)


def test_3d(mg, built):
    n, boxes, ov = [16, 16, 8], [4, 4, 2], [1, 1, 1]
    A, mesh, b = dd_cases.poisson(mg, n, seed=2)
    p = dd_cases.dd_param(mg, A, mesh, boxes, ov)
    info = _info(mg, A, p)
    assert (info["numSub"], info["colours"], info["batched"], info["sequential"]) == (32, 8, 8, 0)
    _check_sweeps(mg, A, b, p, dd_cases.Restated(mg, A, n, boxes, ov))


def test_uneven_boxes(mg, built):
    """34 = 4*8 + 2 and 30 = 4*7 + 2: the last box of a line absorbs the remainder, so one launch holds sub-domains of
    different orders and level counts."""
    n, boxes, ov = [34, 30], [4, 4], [1, 1]
    A, mesh, b = dd_cases.poisson(mg, n, seed=3)
    p = dd_cases.dd_param(mg, A, mesh, boxes, ov)
    assert len({len(g) for g in p.GlobalIndices}) > 2
    info = _info(mg, A, p)
    assert (info["colours"], info["batched"]) == (4, 4)
    _check_sweeps(mg, A, b, p, dd_cases.Restated(mg, A, n, boxes, ov))


def test_dependent_colours_run_in_sequence(mg, built):
    """overlap 2 on cells of 4: boxes of one colour share nodes, a batched update would race."""
    A, mesh, b = dd_cases.poisson(mg, [32, 32], seed=4)
    p = dd_cases.dd_param(mg, A, mesh, [8, 8], [2, 2])
    info = _info(mg, A, p)
    assert (info["colours"], info["batched"], info["sequential"]) == (4, 0, 4)
    assert info["launches_per_sweep"] == 3 * 64
    assert not any(mg.coloursIndependent(A, p).values())
    _check_sweeps(mg, A, b, p, dd_cases.Restated(mg, A, [32, 32], [8, 8], [2, 2]))


@pytest.mark.parametrize("doTranspose", [0, 1])
def test_complex(mg, built, doTranspose):
    A, mesh = helmholtz(mg, [32, 32], 0.5, 0.5)
    b = complex_rhs(A.shape[0])
    p = dd_cases.dd_param(mg, A, mesh, [8, 8], [1, 1], VAL=np.complex128)
    info = _info(mg, A, p)
    assert info["complex"] and (info["colours"], info["batched"]) == (4, 4)
    _check_sweeps(mg, A, b, p, dd_cases.Restated(mg, A, [32, 32], [8, 8], [1, 1]), doTranspose)


def test_real_solver_refuses_complex_operator(mg, built):
    A, mesh = helmholtz(mg, [32, 32], 0.5, 0.5)
    Ainv = mg.ParallelJuliaSolver.getParallelJuliaSolver(np.float64, np.int64)
    p = mg.getDomainDecompositionParam(np.float64, np.int64, mesh, [8, 8], [1, 1], mg.getNodalIndicesOfCell, Ainv)
    with pytest.raises(TypeError):
        mg.setupDDSerial(A, p)
    Ar, mesh, b = dd_cases.reference_case(mg)[:3]
    p = dd_cases.dd_param(mg, Ar, mesh, [8, 8], [1, 1])
    with pytest.raises(TypeError):
        mg.solveDDSerial(A, complex_rhs(A.shape[0]), np.zeros(A.shape[0], dtype=np.complex128), p)


@pytest.mark.parametrize("VAL", [np.float64, np.complex128])
def test_chip_wide_members(mg, built, monkeypatch, VAL):
    """MG_LU_MULTI_MIN_ROWS = 64 makes every sub-domain of the 3-D case (up to 7^3 rows) a large member: residual gather,
    the applier's chip-wide solve, scatter-add, one member after another."""
    monkeypatch.setenv("MG_LU_MULTI_MIN_ROWS", "64")
    n, boxes, ov = [16, 16, 8], [4, 4, 2], [1, 1, 1]
    A, mesh, b = dd_cases.poisson(mg, n, seed=2)
    if VAL is np.complex128:
        A = (A + 0.3j * sp.identity(A.shape[0]) * A.diagonal().max()).tocsr()
        b = complex_rhs(A.shape[0])
    p = dd_cases.dd_param(mg, A, mesh, boxes, ov, VAL=VAL)
    info = _info(mg, A, p)
    assert (info["colours"], info["batched"], info["sequential"]) == (8, 0, 8)
    assert info["launches_per_sweep"] > 3 * 32
    _check_sweeps(mg, A, b, p, dd_cases.Restated(mg, A, n, boxes, ov), doTranspose=1 if VAL is np.complex128 else 0)


def test_device_pointer_form(mg, built):
    import torch
    A, mesh, b, R = dd_cases.reference_case(mg)
    p = dd_cases.dd_param(mg, A, mesh, [8, 8], [1, 1])
    n = A.shape[0]
    buf = torch.full((n + 24,), 7.0, dtype=torch.float64, device="cuda")
    x = buf[11:11 + n]
    x.zero_()
    bd = torch.from_numpy(b).cuda()
    out, _ = mg.solveDDSerial(A, bd, x, p, 1, 0)
    assert out is x
    torch.cuda.synchronize()
    assert _close(x.cpu().numpy(), R.sweep(b, np.zeros_like(b)))
    assert bool((buf[:11] == 7.0).all()) and bool((buf[11 + n:] == 7.0).all())
    assert np.array_equal(bd.cpu().numpy(), b)


def test_preconditioner_in_gmres(mg, built):
    A, mesh, b, R = dd_cases.reference_case(mg)
    p = dd_cases.dd_param(mg, A, mesh, [8, 8], [1, 1])
    x, its = dd_cases.gmres_count(A, b, mg.getDDpreconditioner(A, p, b))
    _, its_ref = dd_cases.gmres_count(A, b, lambda r: R.sweep(r, np.zeros_like(r)))
    print(f"gmres iterations: device preconditioner {its}, restated {its_ref}")
    assert np.linalg.norm(b - A @ x) <= 1e-8 * np.linalg.norm(b)
    assert abs(its - its_ref) <= 1


def test_refusals_leave_the_handle_usable(mg, built):
    A, mesh, b, R = dd_cases.reference_case(mg)
    p = dd_cases.dd_param(mg, A, mesh, [8, 8], [1, 1])
    lib = mg.device.load_library()
    n = A.shape[0]
    a64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
    rp, ci, nz = a64(A.indptr) + 1, a64(A.indices) + 1, np.ascontiguousarray(A.data)
    idxptr = a64(np.concatenate(([0], np.cumsum([len(g) for g in p.GlobalIndices])))) + 1
    idx = np.ascontiguousarray(np.concatenate(p.GlobalIndices), dtype=np.uint32)
    color = a64([mg.cellColor(q.i) for q in p.PrecParams])
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint))
    i64, f64 = mg.device._i64, mg.device._f64

    def create(ix):
        h = C.c_void_p()
        return lib.mg_dd_create_FP64_INT64(0, n, i64(rp), i64(ci), f64(nz), 64, i64(idxptr), u32(ix), i64(color), C.byref(h)), h

    for bad in (0, n + 1):
        ix = idx.copy()
        ix[5] = bad
        rc, h = create(ix)
        assert rc == MG_ERR_INVALID and not h.value
    rc, h = create(idx)
    assert rc == 0
    try:
        def set_factor(ic, s=None):
            s = s or p.PrecParams[ic - 1].Ainv
            Lp, Lc, Lv = a64(s.L.indptr) + 1, a64(s.L.indices) + 1, np.ascontiguousarray(s.L.data)
            Up, Uc, Uv = a64(s.U.indptr) + 1, a64(s.U.indices) + 1, np.ascontiguousarray(s.U.data)
            return lib.mg_dd_set_factor_FP64_INT64(h, ic, s.L.shape[0], i64(Lp), i64(Lc), f64(Lv), i64(Up), i64(Uc), f64(Uv),
                                                   i64(a64(s.p)), i64(a64(s.q)))
        for ic in range(1, 64):
            assert set_factor(ic) == 0
        assert lib.mg_dd_finalize(h) == MG_ERR_STATE                       # sub-domain 64 has no factors yet
        assert set_factor(64, p.PrecParams[9].Ainv) == MG_ERR_INVALID      # an interior box's factors: n_i differs from the corner's list
        assert set_factor(64) == 0
        assert lib.mg_dd_finalize(h) == 0
        x = np.zeros(n)
        z = np.zeros(2 * n)
        assert lib.mg_dd_apply_CFP64(h, f64(z), f64(z.copy()), n, 1, 0) == MG_ERR_STATE
        assert b"Float64" in lib.mg_last_error()
        assert lib.mg_dd_apply_FP64(h, f64(b), f64(x), n + 1, 1, 0) == MG_ERR_INVALID
        assert lib.mg_dd_apply_FP64(h, f64(b), f64(x), n, 1, 0) == 0
        assert _close(x, R.sweep(b, np.zeros_like(b)))
    finally:
        lib.mg_dd_destroy(h)
