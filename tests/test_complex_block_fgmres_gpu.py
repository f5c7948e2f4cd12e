"""-m gpu: complex block FGMRES (mg_block_fgmres[_dev]_CFP64) and its Gram kernels on the MI355X, against numpy and the block oracle
(tests/complex_block_fgmres_oracle.py).

Tolerances are the project's own for the complex block path (tests/test_complex_block_gpu.py): the Gram kernel alone 1e-13 of
||X||_F ||Y||_F (the products' bound; sums of at most 4913 terms of unit-scale data), the first inner step 1e-10, the driver the
oracle's flag, count and resvec length exactly, resvec and X within 1e-8, true residual below 1e-8.  The true residual is the one
block FGMRES controls and tests/test_krylov.py checks for it, ||B - A X||_F / ||B||_F; the worst single column is printed: on
(C1, 4, 10) the ORACLE leaves column 0 at 1.058e-8 with 8.10e-9 over the block, so a per-column bound of 1e-8 is not the method's."""
import ctypes as C

import numpy as np
import pytest
import torch

import complex_block_fgmres_oracle as cf
import complex_block_oracle as cb
import complex_krylov_oracle as ck
import complex_single_oracle as cs
from complex_cases import complex_rhs, helmholtz

pytestmark = pytest.mark.gpu

MG_ERR_INVALID, MG_ERR_STATE, MG_ERR_UNSUPPORTED = 1, 3, 4


@pytest.fixture(scope="module")
def devs(mg, built):
    made = {}

    def get(name, single=False):
        if (name, single) not in made:
            p, As, _ = (cs if single else ck).case(mg, name)
            made[(name, single)] = mg.device.DeviceHierarchy(p)
            made[(name, single)].set_krylov_operator(As)
        return made[(name, single)]

    yield get
    for d in made.values():
        d.close()


# ---- the Gram kernel alone -------------------------------------------------------------------------------------------------------
def _unit_block(rng, n, k):
    return rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k))


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 16])
def test_gram_onepass_against_long_double(mg, devs, k):
    """X^H Y by the one-pass kernel for every lane-group width (k = 3, 5: idle lanes; 16: one group), n = 1, one row short of a tile
    row count, on it, one past it, and 4913 (several workgroups, a ragged last tile), with Y apart from X and Y is X; two runs give
    equal bits; a block on a 16-byte but not 32-byte boundary is served."""
    dev = devs("C3")
    rng = np.random.default_rng(700 + k)
    for n in (1, 63, 64, 65, 4913):
        X, Y = _unit_block(rng, n, k), _unit_block(rng, n, k)
        Xt, Yt = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
        Xl, Yl = X.astype(np.clongdouble), Y.astype(np.clongdouble)
        for tag, At, Bt, ref in (("X^H Y", Xt, Yt, Xl.conj().T @ Yl), ("X^H X", Xt, Xt, Xl.conj().T @ Xl)):
            G = dev.cblk_gram(At, Bt)
            scale = np.linalg.norm(X) * np.linalg.norm(Y if Bt is Yt else X)
            err = float(np.linalg.norm((G - ref).astype(np.complex128))) / scale
            print(f"  k={k} n={n} {tag}: {err:.2e}")
            assert G.shape == (k, k) and err <= 1e-13
            assert np.array_equal(G, dev.cblk_gram(At, Bt))
        # 16 bytes into an allocation: not 32-byte aligned
        base = torch.zeros(2 * n * k + 1, dtype=torch.complex128, device="cuda")
        Xo, Yo = base[1:n * k + 1].view(n, k), base[n * k + 1:].view(n, k)
        Xo.copy_(Xt)
        Yo.copy_(Yt)
        assert Xo.data_ptr() % 32 == 16 and Xo.is_contiguous()
        assert np.array_equal(dev.cblk_gram(Xo, Yo), dev.cblk_gram(Xt, Yt))
        assert np.array_equal(dev.cblk_gram(Xo, Xo), dev.cblk_gram(Xt, Xt))


# ---- the combination kernel through the driver's first inner steps ----------------------------------------------------------------
def _check_run(tag, got, ref, As, B, residual=True):
    X, flag, steps, rv = got
    Xo, fo, so, rvo = ref
    dr = np.abs(rv - rvo[: len(rv)]).max() / rvo[0] if len(rv) else 0.0
    dx = np.abs(X - Xo).max() / np.abs(Xo).max()
    res = np.linalg.norm(B - As @ X) / np.linalg.norm(B)
    col = (np.linalg.norm(B - As @ X, axis=0) / np.linalg.norm(B, axis=0)).max()
    print(f"  {tag}: flag {flag} ({fo}), steps {steps} ({so}), resvec diff {dr:.2e}, X diff {dx:.2e}, true residual {res:.3e} "
          f"(worst column {col:.3e})")
    assert (flag, steps, len(rv)) == (fo, so, len(rvo))
    assert dr <= 1e-8 and dx <= 1e-8
    if residual:
        assert res < 1e-8
    return dr, dx


@pytest.mark.parametrize("inner", [1, 2])
def test_comb_gram_through_the_first_inner_steps(mg, devs, inner):
    """inner = 1, maxIter = 1 on C3, k = 3: one Cholesky QR of R, one inner step, the update of X.  Every combination of that run is
    cx_blk_comb_gram or cx_blk_comb: W -= V_0 H_00 with out == add and Q == out (its epilogue is W^H W), W <- W R1^+ with out == in
    and Q == out.  X and the single resvec entry match the oracle within 1e-10.  inner = 2 adds the epilogue with Q a third block
    (V_1^H W from W -= V_0 H_01)."""
    p, As, _ = ck.case(mg, "C3")
    n, k = As.shape[0], 3
    B = cb.block_rhs(n, k)
    ref = cf.reference(mg, "C3", k, inner, maxIter=1, key="one restart")
    assert (ref[1], ref[2], len(ref[3])) == (-1, inner, inner)
    X = np.zeros((n, k), dtype=np.complex128, order="F")
    got = devs("C3").block_fgmres(B, X, inner, ck.TOL, 1)
    assert got[0] is X
    Xd, flag, steps, rv = got
    dx = np.abs(Xd - ref[0]).max() / np.abs(ref[0]).max()
    dr = np.abs(rv - ref[3]).max() / ref[3][0]
    print(f"  inner {inner}: X diff {dx:.2e}, resvec diff {dr:.2e}")
    assert (flag, steps, len(rv)) == (-1, inner, inner)
    assert dx <= 1e-10 and dr <= 1e-10


# ---- the driver against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,inner", [("C3", 3, 10), ("C1", 2, 5), ("C1", 4, 10), ("C3", 16, 5)])
def test_block_fgmres_against_oracle(mg, devs, name, k, inner):
    p, As, _ = ck.case(mg, name)
    n = As.shape[0]
    B = cb.block_rhs(n, k)
    X = np.zeros((n, k), dtype=np.complex128, order="F")
    got = devs(name).block_fgmres(B, X, inner, ck.TOL, ck.MAXIT_FGMRES)
    assert got[0] is X
    _check_run(f"{name} k={k} inner={inner}", got, cf.reference(mg, name, k, inner), As, B)
    assert (got[2], got[1]) == (cf.BLOCK_FGMRES_RUNS[(name, k, inner)], 0)


def test_block_fgmres_edges_on_c3(mg, devs):
    p, As, _ = ck.case(mg, "C3")
    dev = devs("C3")
    n, k, inner = As.shape[0], 3, 10
    B = cb.block_rhs(n, k)
    zeros = lambda kk=k: np.zeros((n, kk), dtype=np.complex128, order="F")
    run = lambda: dev.block_fgmres(B, zeros(), inner, ck.TOL, ck.MAXIT_FGMRES)
    # B = 0: flag -9, X zero
    X0 = np.asfortranarray(np.stack([complex_rhs(n, 3 + j) for j in range(k)], axis=1))
    X, flag, steps, rv = dev.block_fgmres(np.zeros_like(B), X0, inner, ck.TOL, 10)
    assert flag == -9 and steps == 0 and len(rv) == 0 and not X.any()
    # maxIter exhausted: flag -1, the oracle's prefix
    ref = cf.reference(mg, "C3", k, 5, maxIter=1, key="one restart of five")
    assert (ref[1], ref[2], len(ref[3])) == (-1, 5, 5)
    _check_run("maxIter 1, inner 5", dev.block_fgmres(B, zeros(), 5, ck.TOL, 1), ref, As, B, residual=False)
    full = cf.reference(mg, "C3", k, 5, key="five")
    assert np.abs(ref[3] - full[3][:5]).max() <= 1e-12 * full[3][0]
    # a non-zero X0
    Xs = 0.01 * np.asfortranarray(np.stack([complex_rhs(n, 3 + j) for j in range(k)], axis=1))      # (X0 itself was zeroed above)
    assert Xs.any()
    ref0 = cf.reference(mg, "C3", k, inner, x0=Xs.copy(), key="x0")
    assert ref0[1] == 0 and ref0[3][-1] < 0.96 * ck.TOL and ref0[3][-2] > 1.01 * ck.TOL       # (the guard of the host tests)
    _check_run("X0 != 0", dev.block_fgmres(B, np.asfortranarray(Xs.copy()), inner, ck.TOL, ck.MAXIT_FGMRES), ref0, As, B)
    # two runs are bit-identical; the _dev form on row-major torch blocks equals the host form bit for bit and leaves B untouched
    r1, r2 = run(), run()
    assert np.array_equal(r1[0], r2[0]) and r1[1:3] == r2[1:3] and np.array_equal(r1[3], r2[3])
    Bt = torch.from_numpy(np.ascontiguousarray(B)).cuda()
    Xt = torch.zeros((n, k), dtype=torch.complex128, device="cuda")
    flag, steps, rv = dev.block_fgmres_dev_CFP64(Bt, Xt, inner, ck.TOL, ck.MAXIT_FGMRES)
    assert (flag, steps) == r1[1:3] and np.array_equal(rv, r1[3]) and np.array_equal(Xt.cpu().numpy(), r1[0])
    assert np.array_equal(Bt.cpu().numpy(), B)
    # one column is legal and runs the block code
    b1 = np.asfortranarray(B[:, :1])
    x1, f1, s1, rv1 = dev.block_fgmres(b1, np.zeros_like(b1), 5, ck.TOL, ck.MAXIT_FGMRES)
    _check_run("k = 1", (x1, f1, s1, rv1), cf.reference(mg, "C3", 1, 5), As, b1)
    assert s1 == cf.BLOCK_FGMRES_RUNS[("C3", 1, 5)]
    # block BiCGSTAB and the single-vector FGMRES on the same handle afterwards: the oracle's counts, as before
    got = dev.block_bicgstab(B, zeros(), ck.TOL, ck.MAXIT_BICGSTAB)
    assert (got[2], got[1]) == cb.BLOCK_RUNS[("C3", k)]
    # the public function
    cells, levels, _ = ck.CASES["C3"]                                # (a param of its own: the shared case may not be modified)
    Ah, mesh = helmholtz(mg, [cells] * 3, 0.5, 0.5)
    q = mg.getMGparam(np.complex128, np.int64, levels, 8, ck.MAXIT_FGMRES, ck.TOL, "SPAI", 1.0, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(Ah, mesh, q)
    try:
        X = zeros()
        Xr, qq, steps, rv = mg.solveBlockGMRES_MG_CFP64(As, q, B, X, True, inner)
        assert Xr is X and qq is q and steps == cf.BLOCK_FGMRES_RUNS[("C3", k, inner)] and q.flag == 0 and q.nrhs == 1
        assert np.array_equal(X, r1[0]) and np.array_equal(rv, r1[3]) and rv is q.resvec
    finally:
        mg.clear_(q)
    with pytest.raises(TypeError):
        dev.block_fgmres(B.real.copy(), np.zeros((n, k)), inner, ck.TOL, 3)


def test_block_fgmres_on_a_single_precision_hierarchy(mg, devs):
    """The block driver on a CF32 handle: every Krylov block ComplexF64, the mixed closure on the whole block as M.  Converged, true
    residual below tol; the step count within the margin tests/test_complex_block_gpu.py allows block BiCGSTAB (the larger of 2 and the
    distance between the host runs with the single and the double M)."""
    name, k, inner = "C3", 3, 10
    p, As, _ = cs.case(mg, name)
    n = As.shape[0]
    B = cb.block_rhs(n, k)
    X = np.zeros((n, k), dtype=np.complex128, order="F")
    _, flag, steps, rv = devs(name, True).block_fgmres(B, X, inner, ck.TOL, ck.MAXIT_FGMRES)
    so = cf.reference(mg, name, k, inner, single=True)[2]
    steps_double = cf.BLOCK_FGMRES_RUNS[(name, k, inner)]
    res = np.linalg.norm(B - As @ X) / np.linalg.norm(B)
    print(f"  {name} k={k}: flag {flag}, steps {steps} ({so} on the host with the single M, {steps_double} with the double M), residual {res:.3e}")
    assert flag == 0 and X.dtype == np.complex128 and len(rv) == steps
    assert res < 1e-8
    assert abs(steps - so) <= max(2, abs(so - steps_double))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_block_fgmres_refusals_leave_the_handle_usable(mg, built):
    import coarse_solver_cases as csc
    import complex_coarse_cases as cc
    import complex_oracle as corc
    lib = mg.device.load_library()
    A, mesh = helmholtz(mg, [8, 8, 8], 0.5, 0.5)
    p = mg.getMGparam(np.complex128, np.int64, 2, 8, 8, 1e-10, "Jac", 0.8, 1, 1, "V", "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(A, mesh, p)
    dev = mg.device.DeviceHierarchy(p)
    A8, mesh8 = mg.poisson_shifted([8, 8, 8])
    pr = mg.getMGparam(np.float64, np.int64, 2, 8, 4, 1e-10, "Jac", 0.8, 1, 1, "V")
    mg.MGsetup(A8, mesh8, pr)
    rdev = mg.device.DeviceHierarchy(pr)
    n = A.shape[0]
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    lz = C.c_longlong(0)
    lp = C.byref(lz)
    hb, hx, res = np.zeros(2 * n * 17), np.zeros(2 * n * 17), np.zeros(65 * 2 + 1)

    def refused(rc, code):
        assert rc == code, (rc, lib.mg_last_error())
        assert lib.mg_last_error()

    host = lambda h, nn, nrhs, inner, maxit=2: lib.mg_block_fgmres_CFP64(h, dp(hb), dp(hx), nn, nrhs, inner, 1e-6, maxit, lp, lp, dp(res), lp)
    try:
        hc = dev.handle
        refused(host(hc, n, 0, 5), MG_ERR_INVALID)
        refused(host(hc, n, 17, 5), MG_ERR_UNSUPPORTED)
        refused(host(hc, n, 2, 0), MG_ERR_INVALID)
        refused(host(hc, n, 2, 65), MG_ERR_INVALID)
        refused(host(hc, n + 1, 2, 5), MG_ERR_INVALID)
        refused(host(hc, n, 2, 5, -1), MG_ERR_INVALID)
        refused(host(rdev.handle, A8.shape[0], 2, 5), MG_ERR_STATE)             # a real hierarchy's handle
        good = torch.zeros((n, 2), dtype=torch.complex128, device="cuda")
        base = torch.zeros(4 * n + 1, dtype=torch.float64, device="cuda")
        vp = C.c_void_p
        torch.cuda.synchronize()
        for nrhs, inner, code in ((0, 5, MG_ERR_INVALID), (17, 5, MG_ERR_UNSUPPORTED), (2, 0, MG_ERR_INVALID), (2, 65, MG_ERR_INVALID)):
            refused(lib.mg_block_fgmres_dev_CFP64(hc, vp(good.data_ptr()), vp(good.data_ptr()), n, nrhs, inner, 1e-6, 2, lp, lp, dp(res), lp), code)
        refused(lib.mg_block_fgmres_dev_CFP64(hc, vp(good.data_ptr()), vp(base.data_ptr() + 8), n, 2, 5, 1e-6, 2, lp, lp, dp(res), lp),
                MG_ERR_INVALID)                                                 # 8 bytes off a 16-byte boundary
        refused(lib.mg_cblk_gram_dev_CFP64(vp(good.data_ptr()), vp(good.data_ptr()), n, 17, vp(base.data_ptr()), vp(base.data_ptr()), None),
                MG_ERR_UNSUPPORTED)
        refused(lib.mg_cblk_gram_dev_CFP64(vp(good.data_ptr()), vp(good.data_ptr()), n, 0, vp(base.data_ptr()), vp(base.data_ptr()), None),
                MG_ERR_INVALID)
        torch.cuda.synchronize()
        assert not base.any() and not good.any() and not hx.any()
        # a real block through the Python layer
        with pytest.raises(TypeError):
            dev.block_fgmres(np.ones((n, 2)), np.zeros((n, 2)), 5, 1e-6, 2)
        with pytest.raises(NotImplementedError):
            dev.block_fgmres_dev(good, good, 5, 1e-6, 2)
        # a handle that is not finalized
        d = np.ascontiguousarray(p.relaxPrecs[0], dtype=np.complex128)
        assert lib.mg_set_relax_CF64(hc, 1, dp(d.view(np.float64)), d.size, 1, 1) == 0
        refused(host(hc, n, 2, 5), MG_ERR_STATE)
        assert lib.mg_finalize(hc) == 0
        # the handle still works: a block cycle against the oracle, and a block FGMRES run that converges
        B = np.asfortranarray(np.stack([complex_rhs(n, 80 + j) for j in range(2)], axis=1))
        X = np.zeros((n, 2), dtype=np.complex128, order="F")
        dev.block_cycle(B, X, 1)
        Xo = cb.block_cycle(p, B, np.zeros((n, 2), dtype=np.complex128))
        for j in range(2):
            assert np.abs(X[:, j] - Xo[:, j]).max() <= 1e-12 * np.abs(Xo[:, j]).max()
        X2, flag, steps, rv = dev.block_fgmres(B, np.zeros_like(B), 5, 1e-9, 20)
        assert flag == 0 and np.linalg.norm(B - A @ X2) / np.linalg.norm(B) < 1e-8
    finally:
        dev.close()
        rdev.close()
    # hierarchies that serve one column only: a GMRES coarsest solve, a K-cycle, a Schwarz coarsest solve
    two = lambda nn: (np.zeros(4 * nn), np.zeros(4 * nn))
    pg = cc.hierarchy(mg, "3lev")
    A16, mesh16 = helmholtz(mg, [16, 16, 16], 0.5, 0.5)
    pk = mg.getMGparam(np.complex128, np.int64, 3, 8, 8, 1e-10, "Jac", 0.8, 2, 1, "K", "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(A16, mesh16, pk)
    A2, mesh2 = helmholtz(mg, [32, 32], 0.5, 0.5)
    ps = csc.setup(mg, A2, mesh2, 3, csc.dd_lu(mg, mesh2, [2, 2], [1, 1], np.complex128), np.complex128, "Jac", 0.8, 2, 2, "V", 12, 1e-8)
    for tag, q in (("GMRES coarsest solve", pg), ("K-cycle", pk), ("Schwarz coarsest solve", ps)):
        qdev = mg.device.DeviceHierarchy(q)
        try:
            nn = q.As[0].shape[0]
            b2, x2 = two(nn)
            rc = lib.mg_block_fgmres_CFP64(qdev.handle, dp(b2), dp(x2), nn, 2, 5, 1e-6, 2, lp, lp, dp(res), lp)
            print(f"  {tag}: status {rc}")
            refused(rc, MG_ERR_UNSUPPORTED)
            Bq = np.asfortranarray(np.stack([complex_rhs(nn, 90 + j) for j in range(2)], axis=1))
            if tag != "Schwarz coarsest solve":                                 # (the Python layer has no guard of its own for that one)
                with pytest.raises(NotImplementedError):
                    qdev.block_fgmres(Bq, np.zeros_like(Bq), 5, 1e-6, 2)
                with pytest.raises(NotImplementedError):
                    mg.solveBlockGMRES_MG_CFP64(None, q, Bq, np.zeros_like(Bq), True, 5)
            else:
                with pytest.raises(mg.device.MGDeviceError, match=rf"status {MG_ERR_UNSUPPORTED}\b.*Schwarz"):
                    qdev.block_fgmres(Bq, np.zeros_like(Bq), 5, 1e-6, 2)
            # the handle's single-vector cycle still runs
            b = complex_rhs(nn, 16)
            x = np.zeros_like(b)
            qdev.cycle(b, x, 1)
            assert np.isfinite(x).all() and x.any()
        finally:
            qdev.close()
            mg.clear_(q)
    mg.clear_(p)
