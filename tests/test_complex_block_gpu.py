"""-m gpu: blocks of right-hand sides on complex hierarchies (the mg_block_* entry points) on the MI355X, against scipy and the block
oracle (tests/complex_block_oracle.py).

Tolerances are the project's own for the complex path (tests/test_complex_gpu.py): products 1e-13 relative, one cycle 1e-12, solveMG's
resvec 1e-10; the block driver is held to what tests/test_krylov.py and tests/test_complex_krylov_gpu.py hold theirs to - the
oracle's flag, count and resvec length exactly, resvec and X within 1e-8, true residual below 1e-8; the ComplexF32 cycle to the
bound of tests/test_complex_single_gpu.py (within 64 * 2^-24 of the restatement in the 2-norm)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

import complex_block_oracle as cb
import complex_krylov_oracle as ck
import complex_oracle as corc
import complex_single_oracle as cs
from complex_cases import complex_rhs, helmholtz

pytestmark = pytest.mark.gpu

MG_ERR_INVALID, MG_ERR_STATE, MG_ERR_UNSUPPORTED = 1, 3, 4
U32 = 2.0 ** -24


def _block(n, k, seed):
    return np.asfortranarray(np.stack([complex_rhs(n, seed + j) for j in range(k)], axis=1))


# ---- products --------------------------------------------------------------------------------------------------------------------
def _awkward_operator(n, seed):
    """tests/test_complex_gpu.py's operator: empty rows, rows across the kernel's 1024-entry chunks, one row longer than a chunk."""
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


def _manual_param(mg, A, nc, seed):
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
    p.relaxPrecs = [rng.standard_normal(n) + 1j * rng.standard_normal(n)]
    p.LU = spla.splu(sp.csc_matrix(Ac))
    p.nrhs = 1
    return p


@pytest.fixture(scope="module")
def awkward(mg, built):
    n, nc = 5000, 700
    A = _awkward_operator(n, 3)
    p = _manual_param(mg, A, nc, 7)
    devs = {w: mg.device.DeviceHierarchy(p, options={"force_rowptr64": w}) for w in (0, 1)}
    yield n, nc, A, p, devs
    for d in devs.values():
        d.close()


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 16])
def test_block_spmv_against_scipy(mg, awkward, k, wide):
    """mg_block_spmv_CF64 on A (complex alpha, beta, and beta = 0), R (beta = 0) and P (beta = 1, in place) for every lane-group
    width (k = 3, 5: idle lanes; 16: the cap), both row-pointer widths.  Column permutations and repeated runs are bit-exact."""
    n, nc, A, p, devs = awkward
    dev = devs[wide]
    OP_A, OP_P, OP_R = mg.device.MG_OP_A, mg.device.MG_OP_P, mg.device.MG_OP_R
    X = _block(n, k, 100)
    Y0 = _block(n, k, 200)
    alpha, beta = 0.7 - 1.3j, -0.4 + 0.25j
    Y = Y0.copy(order="F")
    assert dev.block_spmv(1, OP_A, alpha, X, beta, Y) is Y
    ref = beta * Y0 + alpha * (A @ X)
    err = np.abs(Y - ref).max() / np.abs(ref).max()
    print(f"  k={k} wide={wide}: A rel err {err:.2e}")
    assert err <= 1e-13
    Yz = np.full((n, k), np.nan + 0j, order="F")                 # beta = 0: Y is not read
    dev.block_spmv(1, OP_A, alpha, X, 0.0, Yz)
    refz = alpha * (A @ X)
    assert np.abs(Yz - refz).max() <= 1e-13 * np.abs(refz).max()
    # two runs give equal bits; permuting the columns of X permutes the columns of Y bit for bit
    Yz2 = np.zeros((n, k), dtype=np.complex128, order="F")
    dev.block_spmv(1, OP_A, alpha, X, 0.0, Yz2)
    assert np.array_equal(Yz, Yz2)
    perm = np.random.default_rng(k).permutation(k)
    Yp = np.zeros((n, k), dtype=np.complex128, order="F")
    dev.block_spmv(1, OP_A, alpha, np.asfortranarray(X[:, perm]), 0.0, Yp)
    assert np.array_equal(Yp, Yz[:, perm])
    # R and P: real operators on complex blocks
    Bc = np.zeros((nc, k), dtype=np.complex128, order="F")
    dev.block_spmv(1, OP_R, 1.0, X, 0.0, Bc)
    refr = p.Rs[0] @ X
    assert np.abs(Bc - refr).max() <= 1e-13 * np.abs(refr).max()
    Xc = _block(nc, k, 300)
    Xf = Y0.copy(order="F")
    dev.block_spmv(1, OP_P, 1.0, Xc, 1.0, Xf)
    refp = Y0 + p.Ps[0] @ Xc
    assert np.abs(Xf - refp).max() <= 1e-13 * np.abs(refp).max()


# ---- cycle -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def helm16(mg):
    return helmholtz(mg, [16, 16, 16], 0.5, 0.5)


def _param(mg, A, mesh, levels, relax, omega, pre, post, cyc, maxIter=8, tol=1e-10, single=False):
    kw = {"singlePrecision": True} if single else {}
    p = mg.getMGparam(np.complex128, np.int64, levels, 8, maxIter, tol, relax, omega, pre, post, cyc, "NoMUMPS", 0.5, 0.0, **kw)
    mg.MGsetup(A, mesh, p)
    return p


def _columns_close(X, Xo, tol):
    for j in range(X.shape[1]):
        scale = np.abs(Xo[:, j]).max()
        if scale == 0.0:
            assert not X[:, j].any(), j                          # a zero column stays exactly zero
        else:
            assert np.abs(X[:, j] - Xo[:, j]).max() <= tol * scale, (j, np.abs(X[:, j] - Xo[:, j]).max() / scale)


@pytest.mark.parametrize("relax,cyc,sparse_lu", [("Jac", "V", False), ("SPAI", "W", False), ("SPAI", "F", True)])
def test_block_cycle_against_oracle(mg, built, helm16, relax, cyc, sparse_lu):
    """One block cycle from zero and a second from the iterate, k = 3 and 16 with one all-zero column, each column against the
    complex oracle at 1e-12; the host form equals the device form bit for bit; afterwards the single-vector cycle is untouched."""
    A, mesh = helm16
    p = _param(mg, A, mesh, 3, relax, 0.8, 2, 1, cyc)
    n = A.shape[0]
    assert n == 4913
    dev = mg.device.DeviceHierarchy(p)
    try:
        if sparse_lu:
            dev._set_coarse(p, force_sparse=True)
            assert dev.lib.mg_finalize(dev.handle) == 0
        b1 = complex_rhs(n, 9)
        x1 = np.zeros_like(b1)
        dev.cycle(b1, x1, 1)                                     # the single-vector result before any block call
        for k in (3, 16):
            B = _block(n, k, 50)
            B[:, 1] = 0.0                                        # one all-zero column inside the block
            X = np.zeros((n, k), dtype=np.complex128, order="F")
            assert dev.block_cycle(B, X, 1) is X
            Xo = cb.block_cycle(p, B, np.zeros((n, k), dtype=np.complex128))
            _columns_close(X, Xo, 1e-12)
            Xfirst = X.copy(order="F")
            dev.block_cycle(B, X, -1)                            # x != 0: decided for the whole block
            Xo = cb.block_cycle(p, B, Xo)
            _columns_close(X, Xo, 1e-12)
            # the device form on row-major blocks: the same bits, from zero and from the iterate
            Bt = torch.from_numpy(np.ascontiguousarray(B)).cuda()
            Xt = torch.full((n, k), 2.0 - 1j, dtype=torch.complex128, device="cuda")
            dev.block_cycle_dev(Bt, Xt, 1)
            torch.cuda.synchronize()
            assert np.array_equal(Xt.cpu().numpy(), Xfirst)
            dev.block_cycle_dev(Bt, Xt, 0)
            torch.cuda.synchronize()
            assert np.array_equal(Xt.cpu().numpy(), X) and np.array_equal(Bt.cpu().numpy(), B)
        x1b = np.zeros_like(b1)
        dev.cycle(b1, x1b, 1)
        assert np.array_equal(x1b, x1)                           # the bits it gave before the block calls
        xo = corc.recursiveCycle(p, b1, np.zeros_like(b1), 1)
        assert np.abs(x1b - xo).max() <= 1e-12 * np.abs(xo).max()
    finally:
        dev.close()


def test_block_cycle_dev_on_a_single_precision_hierarchy(mg, built, helm16):
    """mg_block_cycle_dev_CFP64 on a CF32 handle: the mixed closure on the whole complex128 block, each column against the
    ComplexF32 restatement within the single cycle's bound (64 * 2^-24 in the 2-norm, tests/test_complex_single_gpu.py), and
    equal bit for bit to the single-vector closure of the same column."""
    A, mesh = helm16
    p = _param(mg, A, mesh, 3, "SPAI", 1.0, 2, 1, "V", single=True)
    n, k = A.shape[0], 3
    dev = mg.device.DeviceHierarchy(p)
    try:
        B = _block(n, k, 60)
        Bt = torch.from_numpy(np.ascontiguousarray(B)).cuda()
        Xt = torch.full((n, k), 1.0 + 1j, dtype=torch.complex128, device="cuda")
        dev.block_cycle_dev(Bt, Xt, 1)
        torch.cuda.synchronize()
        X = Xt.cpu().numpy()
        M = cs.preconditioner(p)
        for j in range(k):
            e = cs.rel2(X[:, j], M(B[:, j]))
            print(f"  column {j}: {e:.3e}")
            assert e < 64 * U32
            bt, xt = torch.from_numpy(np.ascontiguousarray(B[:, j])).cuda(), torch.zeros(n, dtype=torch.complex128, device="cuda")
            dev.cycle_dev(bt, xt, 1)
            torch.cuda.synchronize()
            assert cs.rel2(X[:, j], xt.cpu().numpy()) < 64 * U32
        with pytest.raises(mg.device.MGDeviceError, match=rf"status {MG_ERR_UNSUPPORTED}\b"):
            dev.block_cycle_dev(Bt, Xt, 0)
        with pytest.raises(mg.device.MGDeviceError, match=rf"status {MG_ERR_STATE}\b"):     # the _CF64 host forms serve CF64 handles
            dev.block_cycle(B, np.zeros_like(B), 1)
        Mb = mg.getMultigridPreconditioner(p, B)                 # a complex128 block against a singlePrecision param
        Z = Mb(B)
        assert Z.dtype == np.complex128 and np.array_equal(Z, X)
    finally:
        dev.close()
        mg.clear_(p)


def test_block_solveMG_against_oracle(mg, built, helm16):
    A, mesh = helm16
    p = _param(mg, A, mesh, 3, "SPAI", 1.0, 2, 1, "V", maxIter=30, tol=1e-8)
    n, k = A.shape[0], 3
    B = _block(n, k, 70)
    X = np.zeros((n, k), dtype=np.complex128, order="F")
    _, _, it = mg.solveMG(p, B, X)
    hist = {}
    Xo, ito = cb.solveMG(p, B, np.zeros((n, k), dtype=np.complex128), hist)
    print(f"  {it} cycles ({ito}), resvec diff {np.abs(p.resvec - hist['resvec']).max() / hist['resvec'][0]:.2e}")
    assert it == ito and it < 30
    assert np.abs(p.resvec - hist["resvec"]).max() <= 1e-10 * hist["resvec"][0]
    assert np.linalg.norm(B - A @ X) / np.linalg.norm(B) < p.relativeTol
    assert p.nrhs == 1                                           # the handle's own nrhs did not change
    # the public cycle and product routes take the block too
    Z = np.zeros((n, k), dtype=np.complex128, order="F")
    mg.recursiveCycle(p, B, Z)
    _columns_close(Z, cb.block_cycle(p, B, np.zeros((n, k), dtype=np.complex128)), 1e-12)
    T = np.zeros((n, k), dtype=np.complex128, order="F")
    mg.SpMatMul(p, 1, "A", B, T)
    assert np.abs(T - A @ B).max() <= 1e-13 * np.abs(A @ B).max()
    M = mg.getMultigridPreconditioner(p, B)
    assert np.array_equal(M(B), Z)
    mg.clear_(p)


# ---- block BiCGSTAB --------------------------------------------------------------------------------------------------------------
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


def _check_block_run(tag, got, ref, As, B, residual=True):
    X, flag, it, rv = got
    Xo, fo, ito, rvo = ref
    dr = np.abs(rv - rvo[: len(rv)]).max() / rvo[0] if len(rv) else 0.0
    dx = np.abs(X - Xo).max() / np.abs(Xo).max()
    res = (np.linalg.norm(B - As @ X, axis=0) / np.linalg.norm(B, axis=0)).max()
    print(f"  {tag}: flag {flag} ({fo}), count {it} ({ito}), resvec diff {dr:.2e}, X diff {dx:.2e}, worst true residual {res:.3e}")
    assert (flag, it, len(rv)) == (fo, ito, len(rvo))
    assert dr <= 1e-8 and dx <= 1e-8
    if residual:
        assert res < 1e-8


@pytest.mark.parametrize("name,k", sorted(cb.BLOCK_RUNS))
def test_block_bicgstab_against_oracle(mg, devs, name, k):
    p, As, _ = ck.case(mg, name)
    n = As.shape[0]
    B = cb.block_rhs(n, k)
    X = np.zeros((n, k), dtype=np.complex128, order="F")
    got = devs(name).block_bicgstab(B, X, ck.TOL, ck.MAXIT_BICGSTAB)
    assert got[0] is X
    _check_block_run(f"{name} k={k}", got, cb.reference(mg, name, k), As, B)
    assert (got[2], got[1]) == cb.BLOCK_RUNS[(name, k)]


def test_block_bicgstab_edges_on_c3(mg, devs):
    p, As, _ = ck.case(mg, "C3")
    dev = devs("C3")
    n, k = As.shape[0], 3
    B = cb.block_rhs(n, k)
    run = lambda maxit=ck.MAXIT_BICGSTAB, rhs=B: dev.block_bicgstab(rhs, np.zeros((n, k), dtype=np.complex128, order="F"), ck.TOL, maxit)
    # B = 0: flag -9, X zero
    X, flag, it, rv = dev.block_bicgstab(np.zeros_like(B), _block(n, k, 3), ck.TOL, 10)
    assert flag == -9 and it == 0 and len(rv) == 0 and not X.any()
    # maxIter exhausted: flag -1, the oracle's prefix
    ref = cb.reference(mg, "C3", k, maxIter=3, key="three")
    assert (ref[1], ref[2], len(ref[3])) == (-1, 3, 7)
    _check_block_run("maxIter 3", run(3), ref, As, B, residual=False)
    # two runs are bit-identical; the _dev form on row-major torch blocks equals the host form bit for bit
    r1, r2 = run(), run()
    assert np.array_equal(r1[0], r2[0]) and r1[1:3] == r2[1:3] and np.array_equal(r1[3], r2[3])
    Bt = torch.from_numpy(np.ascontiguousarray(B)).cuda()
    Xt = torch.zeros((n, k), dtype=torch.complex128, device="cuda")
    flag, it, rv = dev.block_bicgstab_dev_CFP64(Bt, Xt, ck.TOL, ck.MAXIT_BICGSTAB)
    assert (flag, it) == r1[1:3] and np.array_equal(rv, r1[3]) and np.array_equal(Xt.cpu().numpy(), r1[0])
    assert np.array_equal(Bt.cpu().numpy(), B)
    # one column is legal and runs the block code
    b1 = np.asfortranarray(B[:, :1])
    x1, f1, i1, rv1 = dev.block_bicgstab(b1, np.zeros_like(b1), ck.TOL, ck.MAXIT_BICGSTAB)
    assert f1 in (0, -3) and np.linalg.norm(b1 - As @ x1) / np.linalg.norm(b1) < 1e-8
    # the public function: nprec = 2 * iter * k + (flag == -3) * k, the handle's nrhs unchanged
    cells, levels, _ = ck.CASES["C3"]                                # (a param of its own: the shared case may not be modified)
    Ah, mesh = helmholtz(mg, [cells] * 3, 0.5, 0.5)
    q = mg.getMGparam(np.complex128, np.int64, levels, 8, ck.MAXIT_BICGSTAB, ck.TOL, "SPAI", 1.0, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(Ah, mesh, q)
    try:
        X = np.zeros((n, k), dtype=np.complex128, order="F")
        Xr, qq, it, nprec = mg.solveBlockBiCGSTAB_MG_CFP64(As, q, B, X)
        assert Xr is X and qq is q and (it, q.flag) == cb.BLOCK_RUNS[("C3", k)]
        assert nprec == 2 * it * k + (q.flag == -3) * k and q.nrhs == 1
        assert np.array_equal(X, r1[0]) and np.array_equal(q.resvec, r1[3])
    finally:
        mg.clear_(q)
    with pytest.raises(TypeError):
        dev.block_bicgstab(B.real.copy(), np.zeros((n, k)), ck.TOL, 3)


@pytest.mark.parametrize("name,k", [("C3", 3), ("C1", 2)])
def test_block_bicgstab_on_a_single_precision_hierarchy(mg, devs, name, k):
    """The block driver on a CF32 handle: every Krylov block ComplexF64, the mixed closure on the whole block as M1.  Converged, true
    residual below tol; the count within the margin the single-vector test allows (tests/test_complex_single_gpu.py: the larger of 2
    and the distance between the host runs with the single and the double M)."""
    p, As, _ = cs.case(mg, name)
    n = As.shape[0]
    B = cb.block_rhs(n, k)
    X = np.zeros((n, k), dtype=np.complex128, order="F")
    _, flag, it, rv = devs(name, True).block_bicgstab(B, X, ck.TOL, ck.MAXIT_BICGSTAB)
    ito = cb.reference(mg, name, k, single=True)[2]
    count_double = cb.BLOCK_RUNS[(name, k)][0]
    res = (np.linalg.norm(B - As @ X, axis=0) / np.linalg.norm(B, axis=0)).max()
    print(f"  {name} k={k}: flag {flag}, count {it} ({ito} on the host with the single M, {count_double} with the double M), residual {res:.3e}")
    assert flag in (0, -3) and X.dtype == np.complex128
    assert res < 1e-8
    assert abs(it - ito) <= max(2, abs(ito - count_double))


def test_block_route_through_the_solver_wrapper(mg, built):
    A, mesh = helmholtz(mg, [16, 16, 16], 0.5, 0.5)
    p = mg.getMGparam(np.complex128, np.int64, 3, 8, 40, 1e-8, "SPAI", 1.0, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
    s = mg.getMGsolver(p, mesh, 0, "BiCGSTAB")
    B = cb.block_rhs(A.shape[0], 3)
    X = np.zeros_like(B)
    mg.solveLinearSystem_(A, B, X, s)
    res = np.linalg.norm(B - A @ X) / np.linalg.norm(B)
    print(f"  ||AX - B||_F / ||B||_F = {res:.3e}, flag {p.flag}")
    assert p.flag in (0, -3) and s.nIter > 0 and res < s.tol
    mg.clear_(p)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_block_refusals_leave_the_handle_usable(mg, built):
    lib = mg.device.load_library()
    A, mesh = helmholtz(mg, [8, 8, 8], 0.5, 0.5)
    p = _param(mg, A, mesh, 2, "Jac", 0.8, 1, 1, "V")
    dev = mg.device.DeviceHierarchy(p)
    A8, mesh8 = mg.poisson_shifted([8, 8, 8])
    pr = mg.getMGparam(np.float64, np.int64, 2, 8, 4, 1e-10, "Jac", 0.8, 1, 1, "V")
    mg.MGsetup(A8, mesh8, pr)
    rdev = mg.device.DeviceHierarchy(pr)
    n = A.shape[0]
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    lz = C.c_longlong(0)
    lp = C.byref(lz)

    def refused(rc, code):
        assert rc == code, (rc, lib.mg_last_error())
        assert lib.mg_last_error()

    try:
        hc, hr = dev.handle, rdev.handle
        hb, hx, ab = np.zeros(2 * n * 17), np.zeros(2 * n * 17), np.zeros(2)
        for nrhs, code in ((0, MG_ERR_INVALID), (17, MG_ERR_UNSUPPORTED)):
            refused(lib.mg_block_cycle_CF64(hc, dp(hb), dp(hx), n, nrhs, 1), code)
            refused(lib.mg_block_solve_CF64(hc, dp(hb), dp(hx), n, nrhs, 1e-6, 2, lp, dp(hb)), code)
            refused(lib.mg_block_spmv_CF64(hc, 1, 0, dp(ab), dp(hb), dp(ab), dp(hx), nrhs), code)
            refused(lib.mg_block_bicgstab_CFP64(hc, dp(hb), dp(hx), n, nrhs, 1e-6, 2, lp, lp, dp(hb), lp), code)
        # a block through an FP64 handle
        refused(lib.mg_block_cycle_CF64(hr, dp(hb), dp(hx), A8.shape[0], 2, 1), MG_ERR_STATE)
        refused(lib.mg_block_bicgstab_CFP64(hr, dp(hb), dp(hx), A8.shape[0], 2, 1e-6, 2, lp, lp, dp(hb), lp), MG_ERR_STATE)
        refused(lib.mg_block_spmv_CF64(hr, 1, 0, dp(ab), dp(hb), dp(ab), dp(hx), 2), MG_ERR_STATE)
        # what stays refused on the complex handle
        refused(lib.mg_cycle_CF64(hc, dp(hb), dp(hx), n, 2, 1), MG_ERR_UNSUPPORTED)
        refused(lib.mg_set_nrhs(hc, 2), MG_ERR_UNSUPPORTED)
        # a misaligned device block (8 bytes off a 16-byte boundary), a wrong n, maxIter < 0, a bad x_is_zero
        base = torch.zeros(4 * n + 1, dtype=torch.float64, device="cuda")
        good = torch.zeros((n, 2), dtype=torch.complex128, device="cuda")
        vp = C.c_void_p
        off = vp(base.data_ptr() + 8)
        torch.cuda.synchronize()
        refused(lib.mg_block_cycle_dev_CFP64(hc, off, vp(good.data_ptr()), n, 2, 1), MG_ERR_INVALID)
        refused(lib.mg_block_bicgstab_dev_CFP64(hc, vp(good.data_ptr()), off, n, 2, 1e-6, 2, lp, lp, dp(hb), lp), MG_ERR_INVALID)
        refused(lib.mg_block_cycle_dev_CFP64(hc, vp(good.data_ptr()), vp(good.data_ptr()), n, 2, 2), MG_ERR_INVALID)
        refused(lib.mg_block_cycle_CF64(hc, dp(hb), dp(hx), n + 1, 2, 1), MG_ERR_INVALID)
        refused(lib.mg_block_bicgstab_CFP64(hc, dp(hb), dp(hx), n, 2, 1e-6, -1, lp, lp, dp(hb), lp), MG_ERR_INVALID)
        torch.cuda.synchronize()
        assert not base.any() and not good.any()
        # a handle that is not finalized
        d = np.ascontiguousarray(p.relaxPrecs[0], dtype=np.complex128)
        assert lib.mg_set_relax_CF64(hc, 1, dp(d.view(np.float64)), d.size, 1, 1) == 0
        refused(lib.mg_block_cycle_CF64(hc, dp(hb), dp(hx), n, 2, 1), MG_ERR_STATE)
        refused(lib.mg_block_bicgstab_CFP64(hc, dp(hb), dp(hx), n, 2, 1e-6, 2, lp, lp, dp(hb), lp), MG_ERR_STATE)
        assert lib.mg_finalize(hc) == 0
        # the Python layer
        with pytest.raises(NotImplementedError):
            dev.block_bicgstab_dev(good, good, 1e-6, 2)
        with pytest.raises(NotImplementedError):
            dev.set_nrhs(2)
        with pytest.raises(NotImplementedError):
            mg.solveGMRES_MG_CFP64(None, p, np.ones((n, 2), dtype=np.complex128, order="F"), np.zeros((n, 2), dtype=np.complex128, order="F"), True, 5)
        # the complex handle still works after all of that: a block cycle and a vector cycle
        B = _block(n, 2, 80)
        X = np.zeros((n, 2), dtype=np.complex128, order="F")
        dev.block_cycle(B, X, 1)
        _columns_close(X, cb.block_cycle(p, B, np.zeros((n, 2), dtype=np.complex128)), 1e-12)
        b = complex_rhs(n, 15)
        x = np.zeros_like(b)
        dev.cycle(b, x, 1)
        xo = corc.recursiveCycle(p, b, np.zeros_like(b), 1)
        assert np.abs(x - xo).max() <= 1e-12 * np.abs(xo).max()
    finally:
        dev.close()
        rdev.close()


def test_block_with_a_schwarz_coarsest_solve_is_refused(mg, built):
    """A Schwarz sweep as coarsest solve (coarse_dd) serves one right-hand side: nrhs = 2 is MG_ERR_UNSUPPORTED, one column runs the
    block code with the sweep, and the handle still matches the restatement's single-vector cycle (the case of
    tests/test_coarse_solver_gpu.py: Helmholtz 32^2 cells, 3 levels, 2 x 2 sub-domains)."""
    import coarse_solver_cases as csc
    A, mesh = helmholtz(mg, [32, 32], 0.5, 0.5)
    boxes, ov = [2, 2], [1, 1]
    p = csc.setup(mg, A, mesh, 3, csc.dd_lu(mg, mesh, boxes, ov, np.complex128), np.complex128, "Jac", 0.8, 2, 2, "V", 12, 1e-8)
    q = csc.oracle_param(p, csc.SweepLU(mg, p, boxes, ov))
    dev = mg.device.DeviceHierarchy(p)
    try:
        assert dev.coarse_form()["kind"] == 4
        n = A.shape[0]
        B = _block(n, 2, 90)
        with pytest.raises(mg.device.MGDeviceError, match=rf"status {MG_ERR_UNSUPPORTED}\b.*Schwarz"):
            dev.block_cycle(B, np.zeros_like(B), 1)
        Bt = torch.from_numpy(np.ascontiguousarray(B)).cuda()
        with pytest.raises(mg.device.MGDeviceError, match=rf"status {MG_ERR_UNSUPPORTED}\b.*Schwarz"):
            dev.block_bicgstab_dev_CFP64(Bt, torch.zeros_like(Bt), 1e-6, 2)
        b = complex_rhs(n, 16)
        xo = corc.recursiveCycle(q, b, np.zeros_like(b), 1)
        x1 = np.zeros((n, 1), dtype=np.complex128, order="F")
        dev.block_cycle(np.asfortranarray(b.reshape(-1, 1)), x1, 1)          # one column is served
        assert np.abs(x1[:, 0] - xo).max() <= 1e-12 * np.abs(xo).max()
        x = np.zeros_like(b)
        dev.cycle(b, x, 1)
        assert np.abs(x - xo).max() <= 1e-12 * np.abs(xo).max()
    finally:
        dev.close()
        mg.clear_(p)
