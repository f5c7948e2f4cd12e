"""-m gpu: ComplexF32 hierarchies on the MI355X - the _CF32 entry points and the ComplexF64 Krylov drivers preconditioned by the
single cycle (the mixed branch) - against the single-precision restatement (tests/complex_single_oracle.py) and the complex128
oracle on the same hierarchy with its values rounded to single.

Bounds.  Stream kernel: per row i with m_i entries, |y_i - ref_i| <= (m_i + 8) 2^-24 (|alpha| sum_k |a_ik||x_k| + |beta||y0_i|) in
moduli against the complex128 product of the single-rounded inputs - each complex product costs at most 2 sqrt(2) units, a sum of m
terms at most m - 1 in any order, the alpha and beta products and the final sum the rest.  Cycle: the device's distance from the
complex128 oracle cycle on rounded(param) is at most 4 e_ref, e_ref the single numpy restatement's distance from the same
comparand - both are the same expression in the same order at unit round-off 2^-24 and differ in FMA contraction and in how the
complex product is formed; a wrong sweep count, a missed conjugation or a wrong level is off by O(1).  Drivers: the host run of the
complex128 oracle drivers with the single restatement as M is the reference; counts within 1 (FGMRES) or max(2, |count with the
single M - count with the double M|) (BiCGSTAB, which amplifies 1e-7 differences in M: no resvec comparison), FGMRES resvec within
1e-4 resvec[0], true residual below 1e-8."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

import complex_krylov_oracle as ck
import complex_oracle as corc
import complex_single_oracle as cs
from complex_cases import complex_rhs, helmholtz
from dd_cases import dd_param

pytestmark = pytest.mark.gpu

MG_ERR_STATE, MG_ERR_UNSUPPORTED = 3, 4
C64 = np.complex64
U32 = 2.0 ** -24


def _single(mg, levels, relax="SPAI", omega=1.0, pre=2, post=1, cyc="V", maxIter=8, tol=1e-6):
    return mg.getMGparam(np.complex128, np.int64, levels, 8, maxIter, tol, relax, omega, pre, post, cyc, "NoMUMPS", 0.5, 0.0,
                         singlePrecision=True)


def _rhs32(n, seed):
    return complex_rhs(n, seed).astype(C64)


# ---- the stream kernel ---------------------------------------------------------------------------------------------------------
def _awkward_operator(n, seed):
    """Complex square CSR (values rounded to single) with empty rows, rows of 400-900 entries across the kernel's 1024-product
    chunks and one row of 3000 entries, longer than a chunk (the single form keeps the chunk of 1024 products)."""
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
    vals = (rng.standard_normal(len(rows)) + 1j * rng.standard_normal(len(rows))).astype(C64)
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    A.sort_indices()
    assert A.dtype == C64
    return A


def _manual_param(mg, A, nc, seed):
    """A two-level ComplexF32 param around an arbitrary A (float32 random P and R, a complex64 coarse operator)."""
    rng = np.random.default_rng(seed)
    n = A.shape[0]
    P = sp.random(n, nc, density=4.0 / nc, random_state=seed, format="csr").astype(np.float32)
    R = sp.random(nc, n, density=6.0 / n, random_state=seed + 1, format="csr").astype(np.float32)
    P.sort_indices()
    R.sort_indices()
    Ac = (sp.identity(nc) * (4.0 + 1j) + 0.1 * sp.random(nc, nc, density=0.05, random_state=seed + 2)).tocsr().astype(C64)
    Ac.sort_indices()
    p = _single(mg, 2, "Jac", 0.8, 1, 1, "V", 4, 1e-6)
    p.As, p.Ps, p.Rs = [A, Ac], [P], [R]
    p.relaxPrecs = [(rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(C64)]
    p.LU = spla.splu(sp.csc_matrix(Ac.astype(np.complex128)))
    p.nrhs = 1
    return p


def _row_bound(M, x, alpha, beta, y0):
    """(m_i + 8) 2^-24 (|alpha| sum_k |a_ik||x_k| + |beta||y0_i|), in double"""
    absM = sp.csr_matrix((np.abs(M.data.astype(np.complex128)), M.indices, M.indptr), shape=M.shape)
    m = np.diff(M.indptr)
    return (m + 8) * U32 * (abs(alpha) * (absM @ np.abs(x.astype(np.complex128))) + abs(beta) * np.abs(y0.astype(np.complex128)))


def _check_rows(tag, y, ref, bound):
    err = np.abs(y.astype(np.complex128) - ref)
    nz = bound > 0
    worst = float((err[nz] / bound[nz]).max())
    print(f"  {tag}: worst row error {worst:.3f} of its bound")
    assert np.all(err[~nz] == 0.0)                              # empty rows with beta = 0 (or y0 = 0): exact
    assert worst <= 1.0, (tag, worst)


@pytest.mark.parametrize("wide", [0, 1])
def test_spmv_cf32_row_bound(mg, built, wide):
    """mg_spmv_CF32 = beta*y + alpha*Op*x for A (complex alpha, beta), R (beta = 0) and P (beta = 1); x and y offset views.
    wide = 1: the 64-bit row-pointer instantiation (option force_rowptr64)."""
    n, nc = 5000, 700
    A = _awkward_operator(n, 3)
    p = _manual_param(mg, A, nc, 7)
    dev = mg.device.DeviceHierarchy(p, options={"force_rowptr64": wide})
    assert isinstance(dev, mg.device.ComplexSingleDeviceHierarchy)
    W = lambda a: a.astype(np.complex128)
    try:
        x = _rhs32(n + 10, 1)[3:3 + n]                           # offset view (not the start of its buffer)
        ybig0 = _rhs32(n + 7, 2)
        alpha, beta = complex(C64(0.7 - 1.3j)), complex(C64(-0.4 + 0.25j))     # (what the float pairs of the call hold)

        def run_A():
            ybig = ybig0.copy()
            dev.spmv(1, mg.device.MG_OP_A, alpha, x, beta, ybig[5:5 + n])
            return ybig

        ybig = run_A()
        y0 = ybig0[5:5 + n]
        ref = beta * W(y0) + alpha * (W(A) @ W(x))
        _check_rows(f"A (rowptr64={wide})", ybig[5:5 + n], ref, _row_bound(A, x, alpha, beta, y0))
        assert np.array_equal(ybig[:5], ybig0[:5]) and np.array_equal(ybig[5 + n:], ybig0[5 + n:])   # nothing outside the view
        assert np.array_equal(run_A(), ybig)                                                         # two runs: the same bits
        xr = _rhs32(n, 4)
        bc = np.zeros(nc, dtype=C64)
        dev.spmv(1, mg.device.MG_OP_R, 1.0, xr, 0.0, bc)
        _check_rows("R", bc, W(p.Rs[0]) @ W(xr), _row_bound(p.Rs[0], xr, 1.0, 0.0, bc))
        xc = _rhs32(nc, 6)
        xf0 = _rhs32(n, 8)
        xf = xf0.copy()
        dev.spmv(1, mg.device.MG_OP_P, 1.0, xc, 1.0, xf)
        _check_rows("P", xf, W(xf0) + W(p.Ps[0]) @ W(xc), _row_bound(p.Ps[0], xc, 1.0, 1.0, xf0))
        with pytest.raises(TypeError):
            dev.spmv(1, mg.device.MG_OP_A, 1.0, W(x), 0.0, W(y0))
    finally:
        dev.close()


# ---- the cycle -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def helm16(mg):
    return helmholtz(mg, [16, 16, 16], 0.5, 0.5)


@pytest.mark.parametrize("relax,cyc,sparse_lu", [("Jac", "V", False), ("SPAI", "W", False), ("SPAI", "F", True),
                                                 ("Jac", "W", True)])
def test_one_cycle_against_the_rounded_double_cycle(mg, built, helm16, relax, cyc, sparse_lu):
    A, mesh = helm16
    p = _single(mg, 3, relax, 0.8, 2, 1, cyc)
    mg.MGsetup(A, mesh, p)
    dev = mg.device.DeviceHierarchy(p)
    try:
        if sparse_lu:                                           # the coarsest solve from the (double) sparse factors
            dev._set_coarse(p, force_sparse=True)
            assert dev.lib.mg_finalize(dev.handle) == 0
        assert dev.coarse_form()["kind"] == (1 if sparse_lu else 0)
        b = _rhs32(A.shape[0], 9)
        pr = cs.rounded(p)
        x = np.zeros_like(b)
        xs = np.zeros_like(b)
        xo = np.zeros(b.shape[0], dtype=np.complex128)
        for k, xz in enumerate((1, -1)):                        # from zero, then from the first iterate (MGcycle.jl:29-31)
            dev.cycle(b, x, xz)
            xs = cs.recursiveCycle(p, b, xs, 1)
            xo = corc.recursiveCycle(pr, b.astype(np.complex128), xo, 1)
            e_ref, e_dev = cs.rel2(xs, xo), cs.rel2(x, xo)
            print(f"  {relax} {cyc} sparse_lu={sparse_lu} cycle {k + 1}: restatement {e_ref:.3e}, device {e_dev:.3e} from the double cycle")
            assert e_ref < 64 * U32
            assert e_dev <= 4 * e_ref
    finally:
        dev.close()


def test_solveMG_single(mg, built, helm16):
    A, mesh = helm16
    p = _single(mg, 3, "SPAI", 1.0, 2, 1, "V", maxIter=12, tol=1e-5)
    mg.MGsetup(A, mesh, p)
    b = _rhs32(A.shape[0], 12)
    try:
        x = np.zeros_like(b)
        _, _, it = mg.solveMG(p, b, x)
        assert x.dtype == C64
        hist = {}
        _, ito = cs.solveMG(p, b, np.zeros_like(b), hist)
        rvo = hist["resvec"]
        x1 = cs.recursiveCycle(p, b, np.zeros_like(b), 1)
        e_ref = cs.rel2(x1, corc.recursiveCycle(cs.rounded(p), b.astype(np.complex128), np.zeros(b.shape[0], dtype=np.complex128), 1))
        tolr = 4 * e_ref * rvo[0]
        k = min(len(rvo), len(p.resvec))
        d = np.abs(p.resvec[:k] - rvo[:k]).max()
        print(f"  solveMG single: {it} cycles ({ito}), resvec diff {d / rvo[0]:.3e} of resvec[0] (allowed {4 * e_ref:.3e}), "
              f"final relres {p.resvec[-1] / p.resvec[0]:.3e}")
        assert d <= tolr
        if abs(rvo[-1] - p.relativeTol * rvo[0]) > tolr:        # (the stopping test is not decided by a rounding)
            assert it == ito
        assert it < 12 and p.resvec[-1] / p.resvec[0] < 1e-5
        with pytest.raises(TypeError):
            mg.solveMG(p, b.astype(np.complex128), np.zeros(b.shape[0], dtype=np.complex128))
        with pytest.raises(TypeError):
            mg.recursiveCycle(p, b.astype(np.complex128), np.zeros(b.shape[0], dtype=np.complex128))
        with pytest.raises(TypeError):
            mg.SpMatMul(p, 1, "A", b.astype(np.complex128), np.zeros(b.shape[0], dtype=np.complex128))
        y = np.zeros_like(b)
        mg.SpMatMul(p, 1, "A", b, y)
        ref = p.As[0].astype(np.complex128) @ b.astype(np.complex128)
        assert cs.rel2(y, ref) < 64 * U32
    finally:
        mg.clear_(p)


# ---- the mixed closure and the drivers -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def devs(mg, built):
    """One ComplexF32 device hierarchy per case with its (ComplexF64) system operator set, shared by the tests below."""
    made = {}

    def get(name):
        if name not in made:
            p, As, _ = cs.case(mg, name)
            made[name] = mg.device.DeviceHierarchy(p)
            made[name].set_krylov_operator(As)
        return made[name]

    yield get
    for d in made.values():
        d.close()


def test_mixed_closure(mg, devs):
    """mg_cycle_dev_CFP64 on a CF32 handle and getMultigridPreconditioner with a complex128 B: widen(single cycle(narrow(b)))."""
    p, As, b = cs.case(mg, "C3")
    dev = devs("C3")
    n = b.shape[0]
    z32 = np.zeros(n, dtype=C64)
    dev.cycle(b.astype(C64), z32, 1)
    want = z32.astype(np.complex128)
    bt, xt = torch.from_numpy(b).cuda(), torch.full((n,), 3.0 + 1j, dtype=torch.complex128, device="cuda")
    dev.cycle_dev(bt, xt, 1)
    torch.cuda.synchronize()
    assert np.array_equal(xt.cpu().numpy(), want) and np.array_equal(bt.cpu().numpy(), b)
    with pytest.raises(mg.device.MGDeviceError, match=rf"status {MG_ERR_UNSUPPORTED}\b"):
        dev.cycle_dev(bt, xt, 0)
    torch.cuda.synchronize()
    assert np.array_equal(xt.cpu().numpy(), want)               # (the refused call wrote nothing)
    e = cs.rel2(want, cs.preconditioner(p)(b))
    print(f"  mixed closure on the device vs the restatement's: {e:.3e}")
    assert e < 64 * U32
    q = _single(mg, 2, "SPAI", 1.0, 2, 1, "V")
    Ah, mesh = helmholtz(mg, [8] * 3, 0.5, 0.5)
    mg.MGsetup(Ah, mesh, q)
    try:
        M = mg.getMultigridPreconditioner(q, b)                 # complex128 B: the mixed closure
        z = M(b)
        assert z.dtype == np.complex128 and np.array_equal(z, want)
        M32 = mg.getMultigridPreconditioner(q, b.astype(C64))   # complex64 B: the plain closure in single
        z = M32(b.astype(C64))
        assert z.dtype == C64 and np.array_equal(z, z32)
        with pytest.raises(TypeError):
            mg.getMultigridPreconditioner(q, b.real.copy())
    finally:
        mg.clear_(q)


def _check_run(tag, got, ref, As, b, method, count_double=None):
    x, flag, it, rv = got
    xo, fo, ito, rvo = ref
    res = np.linalg.norm(b - As @ x) / np.linalg.norm(b)
    k = min(len(rv), len(rvo))
    dr = np.abs(rv[:k] - rvo[:k]).max() / rvo[0] if k else 0.0
    print(f"  {tag}: flag {flag} ({fo}), count {it} ({ito} on the host with the single M, {count_double} with the double M), "
          f"resvec diff {dr:.2e}, true residual {res:.3e}")
    assert flag in (0, -3)
    assert res < 1e-8
    if method == "fgmres":
        assert abs(it - ito) <= 1
        assert dr <= 1e-4
    else:
        assert abs(it - ito) <= max(2, abs(ito - count_double))


@pytest.mark.parametrize("name", ["C1", "C2", "C3"])
def test_bicgstab_mixed(mg, devs, name):
    p, As, b = cs.case(mg, name)
    x = np.zeros_like(b)
    got = devs(name).bicgstab(b, x, ck.TOL, ck.MAXIT_BICGSTAB)
    assert got[0] is x and x.dtype == np.complex128
    _check_run(f"{name} BiCGSTAB", got, cs.reference(mg, name, "bicgstab"), As, b, "bicgstab", ck.EXPECTED[name]["bicgstab"][0])


@pytest.mark.parametrize("name,inner", [("C1", 5), ("C1", 10), ("C2", 10), ("C3", 5), ("C3", 10)])
def test_fgmres_mixed(mg, devs, name, inner):
    p, As, b = cs.case(mg, name)
    x = np.zeros_like(b)
    got = devs(name).fgmres(b, x, inner, ck.TOL, ck.MAXIT_FGMRES)
    _check_run(f"{name} FGMRES({inner})", got, cs.reference(mg, name, "fgmres", inner), As, b, "fgmres", ck.EXPECTED[name][inner])


def test_driver_edges_on_c3(mg, devs):
    p, As, b = cs.case(mg, "C3")
    dev = devs("C3")
    n = b.shape[0]
    run_b = lambda x0, maxit=ck.MAXIT_BICGSTAB, rhs=b: dev.bicgstab(rhs, x0, ck.TOL, maxit)
    run_g = lambda x0, maxit=ck.MAXIT_FGMRES, rhs=b: dev.fgmres(rhs, x0, 5, ck.TOL, maxit)
    for run in (run_b, run_g):                                   # b = 0: flag -9, x zero
        x, flag, it, rv = run(complex_rhs(n, 3), rhs=np.zeros_like(b))
        assert flag == -9 and it == 0 and len(rv) == 0 and not x.any()
    x, flag, it, rv = run_b(np.zeros_like(b), 3)                 # maxIter reached: flag -1
    assert (flag, it, len(rv)) == (-1, 3, 7)
    x, flag, it, rv = run_g(np.zeros_like(b), 3)
    assert (flag, it, len(rv)) == (-1, 15, 15)
    # two runs of each driver are bit-identical; the _dev entry points on torch.complex128 tensors equal them bit for bit
    for run, run_dev in ((run_b, lambda bt, xt: dev.bicgstab_dev(bt, xt, ck.TOL, ck.MAXIT_BICGSTAB)),
                         (run_g, lambda bt, xt: dev.fgmres_dev(bt, xt, 5, ck.TOL, ck.MAXIT_FGMRES))):
        r1, r2 = run(np.zeros_like(b)), run(np.zeros_like(b))
        assert np.array_equal(r1[0], r2[0]) and r1[1:3] == r2[1:3] and np.array_equal(r1[3], r2[3])
        bt, xt = torch.from_numpy(b).cuda(), torch.zeros(n, dtype=torch.complex128, device="cuda")
        flag, it, rv = run_dev(bt, xt)
        assert (flag, it) == r1[1:3] and np.array_equal(rv, r1[3]) and np.array_equal(xt.cpu().numpy(), r1[0])
        assert np.array_equal(bt.cpu().numpy(), b)
    with pytest.raises(TypeError):                               # the Krylov vectors are ComplexF64
        dev.bicgstab(b.astype(C64), np.zeros(n, dtype=C64), ck.TOL, 3)
    with pytest.raises(TypeError):
        dev.fgmres_dev(torch.zeros(n, dtype=torch.complex64, device="cuda"), torch.zeros(n, dtype=torch.complex64, device="cuda"), 5, ck.TOL, 3)
    with pytest.raises(TypeError):
        mg.solveBiCGSTAB_MG_CFP64(As, p, b.astype(C64), np.zeros(n, dtype=C64))


def test_no_krylov_operator_is_the_widened_fine_level(mg, built):
    """Without a Krylov operator the drivers apply As[1] widened to ComplexF64 - the same bits as that matrix uploaded as one."""
    p, As, b = cs.case(mg, "C3")
    dev = mg.device.DeviceHierarchy(p)
    try:
        A0 = p.As[0].astype(np.complex128)
        unset = dev.fgmres(b, np.zeros_like(b), 5, ck.TOL, ck.MAXIT_FGMRES)
        assert unset[1] == 0 and np.linalg.norm(b - A0 @ unset[0]) / np.linalg.norm(b) < 1e-8
        dev.set_krylov_operator(A0)
        as0 = dev.fgmres(b, np.zeros_like(b), 5, ck.TOL, ck.MAXIT_FGMRES)
        dev.set_krylov_operator(None)
        cleared = dev.fgmres(b, np.zeros_like(b), 5, ck.TOL, ck.MAXIT_FGMRES)
        for alt in (as0, cleared):
            assert np.array_equal(unset[0], alt[0]) and unset[1:3] == alt[1:3] and np.array_equal(unset[3], alt[3])
    finally:
        dev.close()


def test_public_route_gmres(mg, built):
    """MGsolver with a single complex param and "GMRES" solves C3's system through solveLinearSystem_ (the hierarchy is set up on the
    operator handed over and rounded to single; the Krylov method runs in double on that rounded operator widened)."""
    _, As, b = cs.case(mg, "C3")
    _, mesh = helmholtz(mg, [ck.CASES["C3"][0]] * 3, 0.5, ck.CASES["C3"][2])
    p = _single(mg, 2, "SPAI", 1.0, 2, 1, "V", maxIter=30, tol=1e-8)
    s = mg.getMGsolver(p, mesh, 2, "GMRES")
    X = np.zeros_like(b)
    try:
        mg.solveLinearSystem_(As, b, X, s)
        assert mg.mgdef.is_single(p) and isinstance(p.device, mg.device.ComplexSingleDeviceHierarchy)
        res = np.linalg.norm(As @ X - b) / np.linalg.norm(b)
        print(f"  GMRES through MGsolver: {s.nIter} steps, flag {p.flag}, ||A X - B|| / ||B|| = {res:.3e}")
        assert p.flag == 0 and s.nIter > 0 and res < 1e-6
    finally:
        mg.clear_(p)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(mg, built):
    lib = mg.device.load_library()
    vp = C.c_void_p
    h = vp()
    assert lib.mg_create_CF32(2, 2, 0, C.byref(h)) == MG_ERR_UNSUPPORTED and lib.mg_last_error()       # two right-hand sides
    A, mesh = helmholtz(mg, [8, 8, 8], 0.5, 0.5)
    ps = _single(mg, 2, "Jac", 0.8, 1, 1, "V")
    pd = mg.getMGparam(np.complex128, np.int64, 2, 8, 8, 1e-6, "Jac", 0.8, 1, 1, "V", "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(A, mesh, ps)
    mg.MGsetup(A, mesh, pd)
    A8, mesh8 = mg.poisson_shifted([8, 8, 8])
    pr = mg.getMGparam(np.float64, np.int64, 2, 8, 4, 1e-10, "Jac", 0.8, 1, 1, "V")
    mg.MGsetup(A8, mesh8, pr)
    sdev, ddev, rdev = mg.device.DeviceHierarchy(ps), mg.device.DeviceHierarchy(pd), mg.device.DeviceHierarchy(pr)
    try:
        hs, hd, hr = sdev.handle, ddev.handle, rdev.handle
        n = A.shape[0]
        bz, xz = np.zeros(2 * n), np.zeros(2 * n)
        bf, xf = np.zeros(2 * n, dtype=np.float32), np.zeros(2 * n, dtype=np.float32)
        dz = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        fz = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_longlong))
        lz = C.c_longlong(0)
        lp = C.byref(lz)

        def refused(rc, code):
            assert rc == code, (rc, code, lib.mg_last_error())
            assert lib.mg_last_error()

        M = ps.As[0]
        cp = np.ascontiguousarray(M.indptr, dtype=np.int64) + 1
        rv = np.ascontiguousarray(M.indices, dtype=np.int64) + 1
        nz32 = np.ascontiguousarray(np.conj(M.data)).view(np.float32)
        nz64 = np.ascontiguousarray(np.conj(pd.As[0].data)).view(np.float64)
        ab32, ab64 = np.zeros(2, dtype=np.float32), np.zeros(2)
        # _CF32 entry points on a CF64 and on an FP64 handle
        for hh in (hd, hr):
            refused(lib.mg_set_operator_CF32_INT64(hh, 1, 0, n, n, ip(cp), ip(rv), fz(nz32)), MG_ERR_STATE)
            refused(lib.mg_set_relax_CF32(hh, 1, fz(bf), n, 1, 1), MG_ERR_STATE)
            refused(lib.mg_cycle_CF32(hh, fz(bf), fz(xf), n, 1, 1), MG_ERR_STATE)
            refused(lib.mg_solve_CF32(hh, fz(bf), fz(xf), n, 1, 1e-6, 2, lp, dz(bz)), MG_ERR_STATE)
            refused(lib.mg_spmv_CF32(hh, 1, 0, fz(ab32), fz(xf), fz(ab32), fz(bf), 1), MG_ERR_STATE)
        # the _CF64 / _FP64 value entry points on the CF32 handle
        refused(lib.mg_set_operator_CF64_INT64(hs, 1, 0, n, n, ip(cp), ip(rv), dz(nz64)), MG_ERR_STATE)
        refused(lib.mg_set_operator_FP64_INT64(hs, 1, 1, n, n, ip(cp), ip(rv), dz(bz)), MG_ERR_STATE)
        refused(lib.mg_set_relax_CF64(hs, 1, dz(bz), n, 1, 1), MG_ERR_STATE)
        refused(lib.mg_cycle_CF64(hs, dz(bz), dz(xz), n, 1, 1), MG_ERR_STATE)
        refused(lib.mg_solve_CF64(hs, dz(bz), dz(xz), n, 1, 1e-6, 2, lp, dz(bz)), MG_ERR_STATE)
        refused(lib.mg_spmv_CF64(hs, 1, 0, dz(ab64), dz(xz), dz(ab64), dz(bz), 1), MG_ERR_STATE)
        refused(lib.mg_cycle_FP64(hs, dz(bz), dz(xz), n, 1, 1), MG_ERR_STATE)
        # what a CF32 handle does not serve
        refused(lib.mg_rap_CF64(hs, dz(nz64), M.nnz, 0, dz(bz), lp), MG_ERR_UNSUPPORTED)
        refused(lib.mg_replace_values_CF64(hs, 1, 0, dz(nz64), M.nnz), MG_ERR_UNSUPPORTED)
        refused(lib.mg_get_values_CF64(hs, 1, 0, dz(nz64), M.nnz), MG_ERR_UNSUPPORTED)
        refused(lib.mg_get_relax_CF64(hs, 1, dz(bz), n), MG_ERR_UNSUPPORTED)
        refused(lib.mg_set_cycle_type(hs, ord("K")), MG_ERR_UNSUPPORTED)
        refused(lib.mg_set_relax_type(hs, 1), MG_ERR_UNSUPPORTED)
        refused(lib.mg_set_nrhs(hs, 2), MG_ERR_UNSUPPORTED)
        refused(lib.mg_cycle_CF32(hs, fz(bf), fz(xf), n, 2, 1), MG_ERR_UNSUPPORTED)
        # a Schwarz coarsest solve: a finalized ComplexF64 sweep handle on the coarsest operator is refused by the CF32 hierarchy
        DD = mg.DomainDecomposition
        Ac = ps.As[-1].astype(np.complex128)
        dd = dd_param(mg, Ac, ps.Meshes[-1], [2, 2, 2], [1, 1, 1], np.complex128)
        try:
            refused(lib.mg_set_coarse_dd(hs, DD._device_handle(dd, Ac)), MG_ERR_UNSUPPORTED)
        finally:
            DD.clear_(dd)
        # the Python layer
        with pytest.raises(NotImplementedError):
            sdev.replace_matrix(ps, ps.As[0])
        with pytest.raises(NotImplementedError):
            sdev.get_values(1, 0)
        with pytest.raises(NotImplementedError):
            sdev.set_nrhs(2)
        with pytest.raises(NotImplementedError):
            sdev.pcg(np.zeros(n, dtype=np.complex128), np.zeros(n, dtype=np.complex128), 1e-6, 3)
        with pytest.raises(TypeError):
            sdev.cycle(np.zeros(n, dtype=np.complex128), np.zeros(n, dtype=np.complex128), 1)
        with pytest.raises(TypeError):
            ddev.cycle(np.zeros(n, dtype=C64), np.zeros(n, dtype=C64), 1)
        for bad, kw in (("cycleType", "K"), ("relaxType", "Jac-GMRES")):
            q = mg.copySolver(ps)
            setattr(q, bad, kw)
            mg.MGsetup(A, mesh, q)
            with pytest.raises(NotImplementedError):
                mg.device.DeviceHierarchy(q)
        q = mg.copySolver(ps)
        q.LU = mg.getDomainDecompositionParam(np.complex128, np.int64, mesh, [2, 2, 2], [1, 1, 1], mg.getNodalIndicesOfCell,
                                              mg.ParallelJuliaSolver.getParallelJuliaSolver(np.complex128, np.int64, numCores=2, backend=1))
        with pytest.raises(NotImplementedError):
            mg.MGsetup(A, mesh, q)
        # the CF32 handle still works after all of that, and a device re-setup request is served by the host path
        b = _rhs32(n, 15)
        x = np.zeros_like(b)
        sdev.cycle(b, x, 1)
        xs = cs.recursiveCycle(ps, b, np.zeros_like(b), 1)
        assert cs.rel2(x, xs) < 64 * U32
    finally:
        sdev.close()
        ddev.close()
        rdev.close()
    A2, _ = helmholtz(mg, [8, 8, 8], 0.5, 0.3)
    ps.device = mg.device.DeviceHierarchy(ps)
    mg.replaceMatrixInHierarchy(ps, A2)                          # host recomputation; the stale device copy is dropped
    assert ps.device is None and ps.As[0].dtype == C64
    b = _rhs32(A2.shape[0], 16)
    x = np.zeros_like(b)
    mg.recursiveCycle(ps, b, x)
    assert cs.rel2(x, cs.recursiveCycle(ps, b, np.zeros_like(b), 1)) < 64 * U32
    mg.clear_(ps)
