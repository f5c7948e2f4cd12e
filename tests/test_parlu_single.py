"""-m gpu: the single-precision factor applier on the MI355X (mg_lu_*_FP32 / _CFP32 behind ParallelJuliaSolver with
``singleFactors=True``, and mg_set_coarse_lu_CF32_INT64 behind a ComplexF32 hierarchy): the reference's own single tests
replayed with its thresholds, the accuracy yardstick of parlu_single_cases against the reference binary in the
single-workgroup and the chip-wide form, the device-pointer entries, misuse, and the hierarchy route.

Yardstick (parlu_single_cases): E is the substitution in double on the single-rounded factors and right-hand sides,
err(X) = max|X - E| / max|E|, and err(device) <= 3 * err(reference binary) on every case: the two differ in the order of
their sums only.  Where no reference run is made (the natural-size case) the comparand is the ComplexF64 applier's solution
on the same rounded factors, rounded to single - the best a single result can be."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import coarse_solver_cases as cs
from complex_cases import helmholtz
from parlu_complex_cases import NRHS, factor, nonsymmetric50
from parlu_single_cases import (FORMS, SOLVE, YARDSTICK, case, create_args, double_substitution, err, lu_form,
                                reference_solution, single_block, single_layout, system)

pytestmark = pytest.mark.gpu

MG_OK, MG_ERR_INVALID, MG_ERR_STATE = 0, 1, 3


def _forms(monkeypatch, multi):
    monkeypatch.setenv("MG_LU_MULTI_MIN_ROWS", "0" if multi else "1000000000")
    monkeypatch.setenv("MG_LU_DENSE_TAIL_MIN", "4")


def _solver(mg, form):
    VAL, IND, _ = FORMS[form]
    return mg.ParallelJuliaSolver.getParallelJuliaSolver(VAL, IND, numCores=2, backend=3, singleFactors=True)


# ---- the reference's own tests ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["FP32_UINT32", "CFP32_UINT32"])
def test_reference_test_replayed_single_laplacians(mg, built, form):
    """testParallelJuliaSolver.jl:56-66 (Float32 / UInt32 on G'*m*G + shift, 20 x 23 cells) and :88-95 (ComplexF32 / UInt32 on
    G'*m*G + (1+1im)*I): one and five right-hand sides converted to single, norm(A x - B, Inf) / norm(B, Inf) < 1e-4; a
    repeated solve gives the same bits."""
    PJ = mg.ParallelJuliaSolver
    VAL = FORMS[form][0]
    rng = np.random.default_rng(0)
    Mr = mg.getRegularMesh([0.0, 1.0, 0.0, 1.0], [20, 23])
    G = mg.getNodalGradientMatrix(Mr)
    m = sp.diags(np.exp(rng.standard_normal(G.shape[0])))
    Ar = (G.T @ m @ G).tocsc()
    N = Ar.shape[1]
    if VAL is np.float32:
        Ar = (Ar + 1e-1 * np.abs(Ar).sum(axis=0).max() * sp.identity(N)).tocsc()
        Bs = (Ar @ rng.random(N), Ar @ rng.random((N, 5)))
    else:
        Ar = (Ar.astype(np.complex128) + (1.0 + 1.0j) * sp.identity(N)).tocsc()
        Bs = (Ar @ (rng.random(N) + 1j * rng.random(N)), Ar @ (rng.random((N, 5)) + 1j * rng.random((N, 5))))
    LU = _solver(mg, form)
    for B in Bs:
        B = np.asfortranarray(B, dtype=VAL)
        x, LU = PJ.solveLinearSystem(Ar, B, LU)
        assert x.dtype == VAL and x.shape == B.shape
        rel = np.abs(Ar @ x.astype(np.complex128) - B).max() / np.abs(B).max()
        print(f"{form} nrhs={1 if B.ndim == 1 else B.shape[1]}: residual {rel:.3e}")
        assert rel < 1e-4
        x2, LU = PJ.solveLinearSystem(Ar, B, LU)
        assert np.array_equal(x, x2)
    assert LU.nFac == 1 and LU.nSolve == 4
    PJ.clear_(LU)


@pytest.mark.parametrize("form", ["FP32_UINT32", "CFP32_UINT32"])
def test_reference_adjoint_sequences_single(mg, built, form):
    """testParallelJuliaSolver.jl:137-150 (Float32 / UInt32) and :167-180 (ComplexF32 / UInt32): the real unsymmetric 50 x 50
    matrix, doTranspose 0, 1, 1, 0, then a block of five with 1, norm(A x - B) / norm(B) < 1e-4; repeated solves give equal
    bits."""
    PJ = mg.ParallelJuliaSolver
    VAL = FORMS[form][0]
    A = nonsymmetric50()
    B, Bs = single_block(form, 50, 1, 31), single_block(form, 50, 5, 35)
    LU = _solver(mg, form)
    X = []
    for t in (0, 1, 1, 0):
        x, LU = PJ.solveLinearSystem(A, B, LU, t)
        Aop = A.T if t else A                                        # (real matrix: A' = A^T)
        rel = np.linalg.norm(Aop @ x.astype(np.complex128) - B) / np.linalg.norm(B)
        print(f"{form} doTranspose={t}: residual {rel:.3e}")
        assert x.dtype == VAL and rel < 1e-4
        X.append(x)
    assert np.array_equal(X[0], X[3]) and np.array_equal(X[1], X[2]) and not np.array_equal(X[0], X[1])
    xs, LU = PJ.solveLinearSystem(A, Bs, LU, 1)
    assert np.linalg.norm(A.T @ xs.astype(np.complex128) - Bs) / np.linalg.norm(Bs) < 1e-4
    assert LU.nFac == 1 and LU.nSolve == 5
    PJ.clear_(LU)


# ---- the yardstick on the 504-row operator whose factor rows are far longer than a wavefront -----------------------------------
@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("form", list(FORMS))
def test_yardstick_plain_and_adjoint(mg, built, form, nrhs, multi, monkeypatch):
    """Plain and adjoint solves in both forms, a lone column, a group of 4 plus 1 and plus 2:
    err(device) <= 3 * err(reference binary)."""
    PJ = mg.ParallelJuliaSolver
    _forms(monkeypatch, multi)
    A = system(form)
    _, F, B, E0 = case(form, nrhs, 0)
    E1 = case(form, nrhs, 1)[3]
    LU = _solver(mg, form)
    X0, LU = PJ.solveLinearSystem(A, B, LU, 0)
    X1, LU = PJ.solveLinearSystem(A, B, LU, 1)
    X0b, LU = PJ.solveLinearSystem(A, B, LU, 0)               # back to the plain factors after an adjoint solve
    assert LU.nFac == 1 and LU.nSolve == 3
    assert np.array_equal(LU.L.data, F["Lv"]) and np.array_equal(LU.U.data, F["Uv"])   # the case's factors are the solver's
    for t in (0, 1):
        f = lu_form(mg, LU._handle, t)
        assert f["kind"] == FORMS[form][2] and f["multi"] == int(multi)
        if multi:
            assert f["tail"] >= 4 and f["launchedL"] < f["levelsL"] and f["launchedU"] < f["levelsU"]
    assert np.array_equal(X0, X0b)
    for t, X, E in ((0, X0, E0), (1, X1, E1)):
        ed, er = err(X, E), err(reference_solution(form, nrhs, t), E)
        print(f"{form} nrhs={nrhs} multi={multi} t={t}: err(device) {ed:.3e}, err(reference) {er:.3e}, ratio {ed / er:.2f}")
        assert ed <= YARDSTICK * er
    if FORMS[form][0] is np.complex64:                        # the adjoint is not the plain transpose
        assert np.abs(A.T @ X1.astype(np.complex128) - B).max() > 1e-3 * np.abs(B).max()
    PJ.clear_(LU)


@pytest.mark.parametrize("multi", [False, True])
def test_uint32_and_int64_handles_give_equal_bits(mg, built, multi, monkeypatch):
    PJ = mg.ParallelJuliaSolver
    _forms(monkeypatch, multi)
    A = system("CFP32_INT64")
    B = case("CFP32_INT64", 5, 0)[2]
    X = {}
    for form in ("CFP32_INT64", "CFP32_UINT32"):
        LU = _solver(mg, form)
        for t in (0, 1):
            X[form, t] = PJ.solveLinearSystem(A, B, LU, t)[0]
        PJ.clear_(LU)
    for t in (0, 1):
        assert np.array_equal(X["CFP32_INT64", t], X["CFP32_UINT32", t])


def test_chip_wide_form_at_a_natural_size(mg, built):
    """Shifted-Laplacian Helmholtz on 96 x 96 cells (9409 rows >= 4096), 16 right-hand sides, no environment switch: the
    chip-wide form with a dense tail is what runs.  err(device) <= 3 * err(X64->32), X64->32 the ComplexF64 applier's
    solution on the same single-rounded factors rounded to single."""
    lib = mg.device.load_library()
    D = mg.device
    A, _ = helmholtz(mg, [96, 96])
    n = A.shape[0]
    assert n == 9409
    F = single_layout(factor(A.tocsc()), "CFP32_INT64")
    B = single_block("CFP32_INT64", n, 16, 5)
    hs, hd = C.c_void_p(), C.c_void_p()
    assert lib.mg_lu_create_CFP32_INT64(0, n, *create_args(mg, F, "CFP32_INT64"), C.byref(hs)) == MG_OK
    Lw, Uw, Bw = F["Lv"].astype(np.complex128), F["Uv"].astype(np.complex128), np.asfortranarray(B, dtype=np.complex128)
    assert lib.mg_lu_create_CFP64_INT64(0, n, D._i64(F["Lp"]), D._i64(F["Lc"]), D._f64(Lw), D._i64(F["Up"]), D._i64(F["Uc"]),
                                        D._f64(Uw), D._i64(F["p"]), D._i64(F["q"]), C.byref(hd)) == MG_OK
    try:
        for t in (0, 1):
            E = double_substitution(F, B, t)
            X, Xw = np.zeros_like(B, order="F"), np.zeros_like(Bw, order="F")
            assert lib.mg_lu_solve_CFP32(hs, D._f32(B), D._f32(X), n, 16, t) == MG_OK
            assert lib.mg_lu_solve_CFP64(hd, D._f64(Bw), D._f64(Xw), n, 16, t) == MG_OK
            f = lu_form(mg, hs, t)
            ed, e64 = err(X, E), err(Xw.astype(np.complex64), E)
            print(f"doTranspose={t}: form {f}, err(device) {ed:.3e}, err(X64->32) {e64:.3e}, ratio {ed / e64:.2f}, "
                  f"ComplexF64 applier against E {err(Xw, E):.3e}")
            assert f["kind"] == 3 and f["multi"] == 1 and f["tail"] > 0
            assert 0 < f["launchedL"] < f["levelsL"] and 0 < f["launchedU"] < f["levelsU"]
            assert ed <= YARDSTICK * e64
    finally:
        assert lib.mg_lu_destroy(hs) == MG_OK and lib.mg_lu_destroy(hd) == MG_OK


# ---- entry points and misuse --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("form", ["CFP32_INT64", "FP32_UINT32"])
def test_device_pointer_entry_equals_host_entry(mg, built, form, multi, monkeypatch):
    import torch
    PJ = mg.ParallelJuliaSolver
    _forms(monkeypatch, multi)
    lib = mg.device.load_library()
    VAL = FORMS[form][0]
    A = system(form)
    n, nrhs = A.shape[0], 5
    B = case(form, nrhs, 0)[2]
    solve_dev = getattr(lib, "mg_lu_solve_dev_" + SOLVE[form])
    LU = _solver(mg, form)
    for t in (0, 1):
        X, LU = PJ.solveLinearSystem(A, B, LU, t)
        bt = torch.from_numpy(np.ascontiguousarray(B).view(np.float32)).cuda()          # row-major [n][nrhs]
        xt = torch.zeros_like(bt)
        torch.cuda.synchronize()
        assert solve_dev(LU._handle, bt.data_ptr(), xt.data_ptr(), n, nrhs, t) == MG_OK
        assert np.array_equal(xt.cpu().numpy().view(VAL), X)
        assert np.array_equal(bt.cpu().numpy().view(VAL), B)                             # b is not work space
    PJ.clear_(LU)


def test_wrong_kind_calls_and_n_equal_one(mg, built):
    lib = mg.device.load_library()
    D = mg.device
    f32, f64 = D._f32, D._f64
    h = {}
    Fs = {}
    for form in ("CFP32_INT64", "FP32_UINT32"):
        Fs[form] = case(form, 1, 0)[1]
        h[form] = C.c_void_p()
        n = Fs[form]["p"].size
        assert getattr(lib, "mg_lu_create_" + form)(0, n, *create_args(mg, Fs[form], form), C.byref(h[form])) == MG_OK
    Fd = Fs["CFP32_INT64"]
    hd = C.c_void_p()
    Lw, Uw = Fd["Lv"].astype(np.complex128), Fd["Uv"].astype(np.complex128)
    assert lib.mg_lu_create_CFP64_INT64(0, n, D._i64(Fd["Lp"]), D._i64(Fd["Lc"]), f64(Lw), D._i64(Fd["Up"]), D._i64(Fd["Uc"]), f64(Uw),
                                        D._i64(Fd["p"]), D._i64(Fd["q"]), C.byref(hd)) == MG_OK
    hc, hr = h["CFP32_INT64"], h["FP32_UINT32"]
    bc, br = case("CFP32_INT64", 1, 0)[2], case("FP32_UINT32", 1, 0)[2]
    xc, xr = np.zeros_like(bc), np.zeros_like(br)
    bd, xd = bc.astype(np.complex128), np.zeros(n, dtype=np.complex128)
    # value-type mix-ups: every solve entry point on every handle of another kind
    assert lib.mg_lu_solve_FP32(hc, f32(br), f32(xr), n, 1, 0) == MG_ERR_STATE and b"ComplexF32" in lib.mg_last_error()
    assert lib.mg_lu_solve_dev_FP32(hc, f32(br), f32(xr), n, 1, 0) == MG_ERR_STATE
    assert lib.mg_lu_solve_CFP32(hr, f32(bc), f32(xc), n, 1, 0) == MG_ERR_STATE and b"Float32" in lib.mg_last_error()
    assert lib.mg_lu_solve_dev_CFP32(hr, f32(bc), f32(xc), n, 1, 1) == MG_ERR_STATE
    assert lib.mg_lu_solve_CFP32(hd, f32(bc), f32(xc), n, 1, 0) == MG_ERR_STATE and b"ComplexF64" in lib.mg_last_error()
    assert lib.mg_lu_solve_CFP64(hc, f64(bd), f64(xd), n, 1, 0) == MG_ERR_STATE and b"ComplexF32" in lib.mg_last_error()
    assert lib.mg_lu_solve_dev_CFP64(hr, f64(bd), f64(xd), n, 1, 0) == MG_ERR_STATE
    assert lib.mg_lu_solve_FP64(hc, f64(bd.real.copy()), f64(xd.real.copy()), n, 1, 0) == MG_ERR_STATE
    assert lib.mg_lu_solve_dev_FP64(hr, f64(bd.real.copy()), f64(xd.real.copy()), n, 1, 0) == MG_ERR_STATE
    # bad arguments
    assert lib.mg_lu_solve_CFP32(hc, f32(bc), f32(xc), n + 1, 1, 0) == MG_ERR_INVALID
    assert lib.mg_lu_solve_CFP32(hc, None, f32(xc), n, 1, 0) == MG_ERR_INVALID
    assert lib.mg_lu_solve_FP32(hr, f32(br), None, n, 1, 0) == MG_ERR_INVALID
    assert lib.mg_lu_solve_FP32(hr, f32(br), f32(xr), n, 0, 0) == MG_ERR_INVALID
    bad = C.c_void_p()
    Fq = dict(Fd, q=Fd["q"] * 0)                                                         # permutation out of range
    assert lib.mg_lu_create_CFP32_INT64(0, n, *create_args(mg, Fq, "CFP32_INT64"), C.byref(bad)) == MG_ERR_INVALID and not bad.value
    assert np.all(xc == 0) and np.all(xr == 0) and np.all(xd == 0)
    # every handle still solves, both directions
    for t in (0, 1, 0):
        assert lib.mg_lu_solve_CFP32(hc, f32(bc), f32(xc), n, 1, t) == MG_OK
        assert err(xc, case("CFP32_INT64", 1, t)[3]) <= YARDSTICK * err(reference_solution("CFP32_INT64", 1, t), case("CFP32_INT64", 1, t)[3])
        assert lib.mg_lu_solve_FP32(hr, f32(br), f32(xr), n, 1, t) == MG_OK
        assert err(xr, case("FP32_UINT32", 1, t)[3]) <= YARDSTICK * err(reference_solution("FP32_UINT32", 1, t), case("FP32_UINT32", 1, t)[3])
        assert lib.mg_lu_solve_CFP64(hd, f64(bd), f64(xd), n, 1, t) == MG_OK
        assert err(xd, case("CFP32_INT64", 1, t)[3]) <= 1e-12
    for hh in (hc, hr, hd):
        assert lib.mg_lu_destroy(hh) == MG_OK
    # n = 1: x = b / (l * u), in double, rounded once
    for form in FORMS:
        VAL, IND, kind = FORMS[form]
        one_p, one_i = np.ones(2, dtype=np.int64) + np.arange(2), np.ones(1, dtype=IND)
        l, u, b = (np.array([v], dtype=VAL) for v in ((1.25 - 0.5j, 3.0 + 0.75j, 0.3 + 0.7j) if VAL is np.complex64 else (1.25, 3.0, 0.3)))
        F1 = dict(Lp=one_p, Lc=one_i, Lv=l, Up=one_p, Uc=one_i, Uv=u, p=one_i, q=one_i)
        h1 = C.c_void_p()
        assert getattr(lib, "mg_lu_create_" + form)(0, 1, *create_args(mg, F1, form), C.byref(h1)) == MG_OK
        assert lu_form(mg, h1)["kind"] == kind
        for t in (0, 1):
            x = np.zeros(1, dtype=VAL)
            assert getattr(lib, "mg_lu_solve_" + SOLVE[form])(h1, f32(b), f32(x), 1, 1, t) == MG_OK
            wide = np.complex128 if VAL is np.complex64 else np.float64
            lw, uw = (l.astype(wide).conj(), u.astype(wide).conj()) if t else (l.astype(wide), u.astype(wide))
            exact = b.astype(wide) / lw / uw
            assert abs(x[0] - exact[0]) <= 2.0 ** -22 * abs(exact[0])      # y and x each rounded once: 2 * 2^-24, and margin 2
        assert lib.mg_lu_destroy(h1) == MG_OK


# ---- the hierarchy route --------------------------------------------------------------------------------------------------------
def _single_param(mg, levels, LU, maxIter=40, tol=1e-8):
    p = mg.getMGparam(np.complex128, np.int64, levels, 8, maxIter, tol, "Jac", 0.8, 2, 2, "V", "NoMUMPS", 0.5, 0.0,
                      singlePrecision=True)
    p.LU = LU
    return p


@pytest.mark.parametrize("multi", [False, True])
def test_one_level_cycle_is_the_solver_objects_solve(mg, built, multi, monkeypatch):
    """A one-level singlePrecision param with a preset single solver object: one cycle is PJ.solve of the same object, bit for
    bit, in both forms - recursiveCycle for a vector, the block closure of getMultigridPreconditioner for a 4-column block."""
    PJ = mg.ParallelJuliaSolver
    _forms(monkeypatch, multi)
    A, mesh = helmholtz(mg, [16, 16], 0.5, 0.5)
    p = _single_param(mg, 1, _solver(mg, "CFP32_INT64"))
    mg.MGsetup(A, mesh, p)
    assert p.LU.singleFactors and p.LU.L.dtype == np.complex64
    n = A.shape[0]
    for nrhs in (1, 4):
        b = single_block("CFP32_INT64", n, nrhs, 40 + nrhs)
        ref = PJ.solve(b, np.zeros_like(b, order="F"), p.LU)
        if nrhs == 1:
            x = np.zeros_like(b)
            mg.recursiveCycle(p, b, x)
        else:
            # (a block on a ComplexF32 hierarchy is served by the mixed closure: one cycle from zero on a ComplexF64 block that is
            #  narrowed and widened in HBM - these values are exactly the single ones)
            bw = b.astype(np.complex128, order="F")
            x = mg.getMultigridPreconditioner(p, bw)(bw)
        assert p.device.coarse_form()["kind"] == (2 if multi else 1)
        assert lu_form(mg, p.LU._handle)["multi"] == int(multi)
        assert np.abs(ref).max() > 0 and np.array_equal(x, ref.astype(x.dtype))
    mg.clear_(p)


def test_two_level_single_hierarchy_with_a_single_solver_object(mg, built):
    """ComplexF32 two-level hierarchy on 32 x 32 cells.  d0: the distance between today's ComplexF32 cycle (ComplexF64 solver
    object, widened coarsest solve) and the ComplexF64 cycle; the new route's distance to the ComplexF64 cycle is at most
    3 * d0, and FGMRES to 1e-8 needs the step count of the ComplexF64-object route +- 1.  Then copySolver, destroyCoarsestLU
    and replaceMatrixInHierarchy on the param."""
    PJ = mg.ParallelJuliaSolver
    A, mesh = helmholtz(mg, [32, 32], 0.5, 0.5)
    n = A.shape[0]
    b = single_block("CFP32_INT64", n, 1, 9)
    p64 = cs.setup(mg, A, mesh, 2, cs.pjs_lu(mg, np.complex128), np.complex128, "Jac", 0.8, 2, 2, "V")
    pold = _single_param(mg, 2, cs.pjs_lu(mg, np.complex128))
    pnew = _single_param(mg, 2, _solver(mg, "CFP32_INT64"))
    mg.MGsetup(A, mesh, pold)
    mg.MGsetup(A, mesh, pnew)
    x64 = np.zeros(n, dtype=np.complex128)
    mg.recursiveCycle(p64, b.astype(np.complex128), x64)
    xo, xn = np.zeros_like(b), np.zeros_like(b)
    mg.recursiveCycle(pold, b, xo)
    mg.recursiveCycle(pnew, b, xn)
    rel = lambda x: float(np.linalg.norm(x.astype(np.complex128) - x64) / np.linalg.norm(x64))
    d0, d1 = rel(xo), rel(xn)
    print(f"cycle distance to ComplexF64: ComplexF64-object route {d0:.3e}, ComplexF32-object route {d1:.3e}")
    assert pnew.device.coarse_form()["kind"] == 1 and pold.device.coarse_form()["kind"] == 1
    assert 0 < d0 < 1e-5 and d1 <= 3 * d0
    steps = {}
    bw = b.astype(np.complex128)
    for name, p in (("old", pold), ("new", pnew)):
        x = np.zeros(n, dtype=np.complex128)
        _, _, _, resvec = mg.solveGMRES_MG_CFP64(A, p, bw, x, True, 20)
        steps[name] = len(resvec)
        assert np.linalg.norm(A @ x - bw) <= 1e-8 * np.linalg.norm(bw) * 1.01
    print(f"FGMRES steps to 1e-8: ComplexF64-object route {steps['old']}, ComplexF32-object route {steps['new']}")
    assert abs(steps["new"] - steps["old"]) <= 1
    # copySolver carries the single solver object; the copy sets up and cycles to the same bits
    c = mg.copySolver(pnew)
    assert c.LU is not pnew.LU and c.LU.singleFactors and np.dtype(c.LU.VAL) == np.complex64
    mg.MGsetup(A, mesh, c)
    xc = np.zeros_like(b)
    mg.recursiveCycle(c, b, xc)
    assert np.array_equal(xc, xn)
    mg.clear_(c)
    # replaceMatrixInHierarchy re-factorises on the host and sets the factors again
    A2, _ = helmholtz(mg, [32, 32], 0.5, 0.3)
    fresh = _single_param(mg, 2, _solver(mg, "CFP32_INT64"))
    mg.MGsetup(A2, mesh, fresh)
    mg.replaceMatrixInHierarchy(pnew, A2)
    assert pnew.LU.singleFactors and pnew.LU.L.dtype == np.complex64
    xr, xf = np.zeros_like(b), np.zeros_like(b)
    mg.recursiveCycle(pnew, b, xr)
    mg.recursiveCycle(fresh, b, xf)
    assert not np.array_equal(xr, xn) and cs.relmax(xr, xf) <= 64 * 2.0 ** -24
    # destroyCoarsestLU clears the object and keeps it
    LU = pnew.LU
    mg.destroyCoarsestLU(pnew)
    assert pnew.LU is LU and LU.L is None and LU._handle is None and pnew.device is None
    # a ComplexF32 object on a ComplexF64 param is the existing value-type TypeError
    with pytest.raises(TypeError):
        cs.setup(mg, A, mesh, 2, _solver(mg, "CFP32_INT64"), np.complex128)
    for q in (p64, pold, pnew, fresh):
        mg.clear_(q)


def test_set_coarse_lu_cf32_is_refused_on_other_handles(mg, built):
    lib = mg.device.load_library()
    D = mg.device
    F = case("CFP32_INT64", 1, 0)[1]
    n = F["p"].size
    args = (n, D._i64(F["Lp"]), D._i64(F["Lc"]), D._f32(F["Lv"]), D._i64(F["Up"]), D._i64(F["Uc"]), D._f32(F["Uv"]), D._i64(F["p"]),
            D._i64(F["q"]))
    for create in (lib.mg_create_CF64, lib.mg_create):
        h = C.c_void_p()
        assert create(1, 1, 0, C.byref(h)) == MG_OK
        assert lib.mg_set_coarse_lu_CF32_INT64(h, *args) in (MG_ERR_STATE, 4)          # (4: MG_ERR_UNSUPPORTED)
        assert lib.mg_destroy(h) == MG_OK
    h = C.c_void_p()
    assert lib.mg_create_CF32(1, 1, 0, C.byref(h)) == MG_OK
    assert lib.mg_set_coarse_lu_CF32_INT64(h, *args) == MG_OK
    assert lib.mg_set_coarse_lu_CF32_INT64(h, n, None, *args[2:]) == MG_ERR_INVALID
    assert lib.mg_destroy(h) == MG_OK
