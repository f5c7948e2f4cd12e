"""-m gpu: the ComplexF64 factor applier on the MI355X (mg_lu_*_CFP64 behind ParallelJuliaSolver with VAL = ComplexF64):
the reference's own complex tests replayed, plain and adjoint solves against scipy and the reference binary in the
single-workgroup and the chip-wide form, the device-pointer entry, refusals.

Tolerances are those of the real applier (tests/test_parallel_julia_solver.py): solutions within 1e-12 * max|X| of scipy
and of the reference binary, residuals within 1e-10 * max|B|; the reference's own replayed tests keep its thresholds."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from complex_cases import helmholtz, lu_layout
from parlu_complex_cases import (NRHS, complex_block, factor, helmholtz_unsymmetric, nonsymmetric50, reference_solution,
                                 shifted_laplacian)

pytestmark = pytest.mark.gpu

MG_OK, MG_ERR_INVALID, MG_ERR_STATE = 0, 1, 3


def _form(mg, LU, t=0):
    info = np.zeros(7, dtype=np.int64)
    lib = mg.device.load_library()
    assert lib.mg_lu_form(LU._handle, t, mg.device._i64(info)) == MG_OK
    return dict(complex=int(info[0]), multi=int(info[1]), tail=int(info[2]), launchedL=int(info[3]), launchedU=int(info[4]),
                levelsL=int(info[5]), levelsU=int(info[6]))


def test_reference_test_replayed_complex_shifted_laplacian(mg, built):
    """testParallelJuliaSolver.jl:72-88: G'*m*G + (1+1im)*I on 20 x 23 cells, one and five right-hand sides, backend 3,
    norm(A x - B, Inf) / norm(B, Inf) < 1e-10."""
    PJ = mg.ParallelJuliaSolver
    Ar = shifted_laplacian(mg)
    N = Ar.shape[1]
    rng = np.random.default_rng(1)
    Bs = (Ar @ (rng.random(N) + 1j * rng.random(N)), np.asfortranarray(Ar @ (rng.random((N, 5)) + 1j * rng.random((N, 5)))))
    LU = PJ.getParallelJuliaSolver(np.complex128, np.int64, numCores=2, backend=3)
    for B in Bs:
        x, LU = PJ.solveLinearSystem(Ar, B, LU)
        assert x.dtype == np.complex128 and x.shape == B.shape
        rel = np.abs(Ar @ x - B).max() / np.abs(B).max()
        print(f"nrhs={1 if B.ndim == 1 else B.shape[1]}: residual {rel:.3e}")
        assert rel < 1e-10
    assert LU.nFac == 1 and LU.nSolve == 2
    PJ.clear_(LU)


def test_reference_adjoint_sequence_real_matrix_complex_solver(mg, built):
    """testParallelJuliaSolver.jl:152-165: a real unsymmetric 50 x 50 matrix through a ComplexF64 solver, doTranspose
    0, 1, 1, 0, then a block of five with 1."""
    PJ = mg.ParallelJuliaSolver
    A = nonsymmetric50()
    assert A.dtype == np.float64 and abs(A - A.T).max() > 0.1
    B, Bs = complex_block(50, 1, 31), complex_block(50, 5, 35)
    lu = factor(A.astype(np.complex128))
    LU = PJ.getParallelJuliaSolver(np.complex128, np.int64, numCores=2, backend=3)
    X = []
    for t in (0, 1, 1, 0):
        x, LU = PJ.solveLinearSystem(A, B, LU, t)
        Aop = A.T if t else A                                        # (real matrix: A' = A^T)
        ref = lu.solve(B, trans="H" if t else "N")
        print(f"doTranspose={t}: residual {np.abs(Aop @ x - B).max() / np.abs(B).max():.3e}, "
              f"vs scipy {np.abs(x - ref).max() / np.abs(ref).max():.3e}")
        assert np.abs(Aop @ x - B).max() <= 1e-10 * np.abs(B).max()
        assert np.abs(x - ref).max() <= 1e-12 * np.abs(ref).max()
        assert np.abs(x - reference_solution(f"nonsym50_nrhs1_t{t}", lu, B, t)).max() <= 1e-12 * np.abs(x).max()
        X.append(x)
    assert np.array_equal(X[0], X[3]) and np.array_equal(X[1], X[2])
    xs, LU = PJ.solveLinearSystem(A, Bs, LU, 1)
    assert np.abs(A.T @ xs - Bs).max() <= 1e-10 * np.abs(Bs).max()
    assert np.abs(xs - lu.solve(Bs, trans="H")).max() <= 1e-12 * np.abs(xs).max()
    assert np.abs(xs - reference_solution("nonsym50_nrhs5_t1", lu, Bs, 1)).max() <= 1e-12 * np.abs(xs).max()
    assert LU.nFac == 1 and LU.nSolve == 5
    PJ.clear_(LU)


@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("nrhs", NRHS)
def test_plain_and_adjoint_solve_complex_unsymmetric(mg, built, nrhs, multi, monkeypatch):
    """x[q] = U\\(L\\b[p]) and, with doTranspose, x[p] = L^H\\(U^H\\b[q]) where A, A^T and A^H all differ, against scipy and
    the reference's applyLUsolve_CFP64_INT64 (its stored outputs where it is not built); `multi` forces the chip-wide form
    and a small dense tail."""
    PJ = mg.ParallelJuliaSolver
    monkeypatch.setenv("MG_LU_MULTI_MIN_ROWS", "0" if multi else "1000000000")
    monkeypatch.setenv("MG_LU_DENSE_TAIL_MIN", "4")
    A = helmholtz_unsymmetric()
    AH = A.conj().T.tocsc()
    assert abs(A - A.T).max() > 1e-2 and abs(A.T - AH).max() > 1e-2
    B = complex_block(A.shape[0], nrhs, 11 + nrhs)
    lu = factor(A)
    LU = PJ.getParallelJuliaSolver(np.complex128, np.int64, numCores=2, backend=3)
    X0, LU = PJ.solveLinearSystem(A, B, LU, 0)
    X1, LU = PJ.solveLinearSystem(A, B, LU, 1)
    X0b, LU = PJ.solveLinearSystem(A, B, LU, 0)               # back to the plain factors after an adjoint solve
    assert LU.nFac == 1 and LU.nSolve == 3
    for t in (0, 1):
        f = _form(mg, LU, t)
        assert f["complex"] == 1 and f["multi"] == int(multi)
        if multi:
            assert f["tail"] >= 4 and f["launchedL"] < f["levelsL"] and f["launchedU"] < f["levelsU"]
    assert np.array_equal(X0, X0b)
    r0, r1 = np.abs(A @ X0 - B).max() / np.abs(B).max(), np.abs(AH @ X1 - B).max() / np.abs(B).max()
    S0, S1 = lu.solve(B), lu.solve(B, trans="H")
    R0 = reference_solution(f"helmholtz_unsym_nrhs{nrhs}_t0", lu, B, 0)
    R1 = reference_solution(f"helmholtz_unsym_nrhs{nrhs}_t1", lu, B, 1)
    e = [np.abs(X0 - S0).max() / np.abs(X0).max(), np.abs(X1 - S1).max() / np.abs(X1).max(),
         np.abs(X0 - R0).max() / np.abs(X0).max(), np.abs(X1 - R1).max() / np.abs(X1).max()]
    print(f"nrhs={nrhs} multi={multi}: residuals {r0:.3e} {r1:.3e}; vs scipy {e[0]:.3e} {e[1]:.3e}; vs reference {e[2]:.3e} {e[3]:.3e}")
    assert r0 <= 1e-10 and r1 <= 1e-10                          # the adjoint residual against A^H ...
    assert np.abs(A.T @ X1 - B).max() > 1e-3 * np.abs(B).max()  # ... which a plain transpose would not pass
    assert max(e) <= 1e-12
    PJ.clear_(LU)


def test_chip_wide_form_at_a_natural_size(mg, built):
    """2-D shifted-Laplacian Helmholtz on 256 x 256 cells, 16 right-hand sides, no environment switch: the chip-wide form
    with a dense tail is what runs, plain and adjoint against scipy."""
    PJ = mg.ParallelJuliaSolver
    A, _ = helmholtz(mg, [256, 256])
    A = A.tocsc()
    B = complex_block(A.shape[0], 16, 5)
    lu = factor(A)
    LU = PJ.getParallelJuliaSolver(np.complex128, np.int64, numCores=2, backend=3)
    for t in (0, 1):
        X, LU = PJ.solveLinearSystem(A, B, LU, t)
        f = _form(mg, LU, t)
        Aop = A.conj().T if t else A
        S = lu.solve(B, trans="H" if t else "N")
        r, e = np.abs(Aop @ X - B).max() / np.abs(B).max(), np.abs(X - S).max() / np.abs(S).max()
        print(f"doTranspose={t}: form {f}, residual {r:.3e}, vs scipy {e:.3e}")
        assert f["complex"] == 1 and f["multi"] == 1 and f["tail"] > 0
        assert 0 < f["launchedL"] < f["levelsL"] and 0 < f["launchedU"] < f["levelsU"]
        assert r <= 1e-10 and e <= 1e-12
    assert LU.nFac == 1 and LU.nSolve == 2
    PJ.clear_(LU)


@pytest.mark.parametrize("multi", [False, True])
def test_device_pointer_entry_equals_host_entry(mg, built, multi, monkeypatch):
    import torch
    PJ = mg.ParallelJuliaSolver
    monkeypatch.setenv("MG_LU_MULTI_MIN_ROWS", "0" if multi else "1000000000")
    monkeypatch.setenv("MG_LU_DENSE_TAIL_MIN", "4")
    lib = mg.device.load_library()
    A = helmholtz_unsymmetric()
    n, nrhs = A.shape[0], 5
    B = complex_block(n, nrhs, 16)
    LU = PJ.getParallelJuliaSolver(np.complex128, np.int64, numCores=2, backend=3)
    for t in (0, 1):
        X, LU = PJ.solveLinearSystem(A, B, LU, t)
        bt = torch.from_numpy(np.ascontiguousarray(B).view(np.float64)).cuda()          # row-major [n][nrhs] (re, im)
        xt = torch.zeros_like(bt)
        torch.cuda.synchronize()
        assert lib.mg_lu_solve_dev_CFP64(LU._handle, bt.data_ptr(), xt.data_ptr(), n, nrhs, t) == MG_OK
        Xd = xt.cpu().numpy().view(np.complex128)
        assert np.array_equal(Xd, X)
        assert np.array_equal(bt.cpu().numpy().view(np.complex128), B)                    # b is not work space
    PJ.clear_(LU)


def test_refusals_and_mixed_use(mg, built):
    lib = mg.device.load_library()
    I, F = mg.device._i64, mg.device._f64
    A = helmholtz_unsymmetric()
    n = A.shape[0]
    luc = factor(A)
    lur = factor(sp.csc_matrix((np.ascontiguousarray(A.data.real), A.indices, A.indptr), shape=A.shape))   # real part, same pattern
    Fc = lu_layout(luc)
    Fr = lu_layout(lur)
    Fr["Lv"], Fr["Uv"] = np.ascontiguousarray(Fr["Lv"].real), np.ascontiguousarray(Fr["Uv"].real)
    hc, hr = C.c_void_p(), C.c_void_p()
    args = lambda G: (0, n, I(G["Lp"]), I(G["Lc"]), F(G["Lv"]), I(G["Up"]), I(G["Uc"]), F(G["Uv"]), I(G["p"]), I(G["q"]))
    assert lib.mg_lu_create_CFP64_INT64(*args(Fc), C.byref(hc)) == MG_OK
    assert lib.mg_lu_create_FP64_INT64(*args(Fr), C.byref(hr)) == MG_OK
    bc, xc = complex_block(n, 1, 2), np.zeros(n, dtype=np.complex128)
    br, xr = bc.real.copy(), np.zeros(n)
    # value-type mix-ups
    assert lib.mg_lu_solve_FP64(hc, F(br), F(xr), n, 1, 0) == MG_ERR_STATE and b"ComplexF64" in lib.mg_last_error()
    assert lib.mg_lu_solve_dev_FP64(hc, F(br), F(xr), n, 1, 0) == MG_ERR_STATE
    assert lib.mg_lu_solve_CFP64(hr, F(bc), F(xc), n, 1, 0) == MG_ERR_STATE and b"Float64" in lib.mg_last_error()
    assert lib.mg_lu_solve_dev_CFP64(hr, F(bc), F(xc), n, 1, 1) == MG_ERR_STATE
    # bad arguments
    assert lib.mg_lu_solve_CFP64(hc, F(bc), F(xc), n + 1, 1, 0) == MG_ERR_INVALID
    assert lib.mg_lu_solve_CFP64(hc, None, F(xc), n, 1, 0) == MG_ERR_INVALID
    assert lib.mg_lu_solve_CFP64(hc, F(bc), None, n, 1, 0) == MG_ERR_INVALID
    assert lib.mg_lu_solve_CFP64(hc, F(bc), F(xc), n, 0, 0) == MG_ERR_INVALID
    assert lib.mg_lu_solve_dev_CFP64(hc, None, None, n, 1, 0) == MG_ERR_INVALID
    assert lib.mg_lu_solve_CFP64(None, F(bc), F(xc), n, 1, 0) == MG_ERR_INVALID
    bad = C.c_void_p()
    Fz = dict(Fc, Lp=Fc["Lp"] - 1, Up=Fc["Up"] - 1)                                     # 0-based row pointers
    assert lib.mg_lu_create_CFP64_INT64(*args(Fz), C.byref(bad)) == MG_ERR_INVALID and not bad.value
    assert lib.mg_lu_create_CFP64_INT64(0, n, None, *args(Fc)[3:], C.byref(bad)) == MG_ERR_INVALID
    Fq = dict(Fc, q=Fc["q"] * 0)                                                         # permutation out of range
    assert lib.mg_lu_create_CFP64_INT64(*args(Fq), C.byref(bad)) == MG_ERR_INVALID and not bad.value
    assert np.all(xc == 0) and np.all(xr == 0)
    # both handles still solve, both directions
    for t, tr in ((0, "N"), (1, "H"), (0, "N")):
        assert lib.mg_lu_solve_CFP64(hc, F(bc), F(xc), n, 1, t) == MG_OK
        ref = luc.solve(bc, trans=tr)
        assert np.abs(xc - ref).max() <= 1e-12 * np.abs(ref).max()
        assert lib.mg_lu_solve_FP64(hr, F(br), F(xr), n, 1, t) == MG_OK
        ref = lur.solve(br, trans="T" if t else "N")
        assert np.abs(xr - ref).max() <= 1e-12 * np.abs(ref).max()
    assert lib.mg_lu_destroy(hc) == MG_OK and lib.mg_lu_destroy(hr) == MG_OK
