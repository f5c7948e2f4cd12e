"""-m gpu: ComplexF64 hierarchies on the MI355X through the _CF64 entry points, against scipy and the complex oracle
(tests/complex_oracle.py) on the same host-built hierarchy, relaxation vectors and coarse factors.

Tolerances: kernel-level products within 1e-13 relative (in-row sums in stored order, products reassociated by the
compiler's FMA contraction only); one cycle within 1e-12; solveMG's resvec within 1e-10 (BASELINE.json north_star)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import complex_oracle as corc
from complex_cases import complex_rhs, helmholtz
from oracle import mg_oracle as orc

pytestmark = pytest.mark.gpu

MG_ERR_STATE, MG_ERR_UNSUPPORTED = 3, 4


def _param(mg, A, mesh, levels, relax="SPAI", omega=1.0, pre=2, post=1, cyc="V", maxIter=8, tol=1e-10):
    p = mg.getMGparam(np.complex128, np.int64, levels, 8, maxIter, tol, relax, omega, pre, post, cyc, "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(A, mesh, p)
    return p


def _awkward_operator(n, seed):
    """Complex square CSR with empty rows, rows spanning the kernel's 1024-entry chunks and one row longer than a chunk."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 12, n)
    lens[rng.choice(n, 40, replace=False)] = 0                 # empty rows
    lens[100:104] = [700, 650, 900, 400]                       # a few long rows: blocks of one or two rows, chunk boundaries
    lens[2000] = 3000                                          # longer than a chunk: the one-long-row branch
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
    """A two-level complex param around an arbitrary A (real random P and R, a complex coarse operator)."""
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


@pytest.mark.parametrize("wide", [0, 1])
def test_spmv_cf64_against_scipy(mg, built, wide):
    """mg_spmv_CF64 = beta*y + alpha*Op*x for A (complex alpha, beta), R and P (real operators, complex vectors); x and y offset
    views of larger arrays.  wide = 1: the 64-bit row-pointer instantiation (option force_rowptr64)."""
    n, nc = 5000, 700
    A = _awkward_operator(n, 3)
    p = _manual_param(mg, A, nc, 7)
    dev = mg.device.DeviceHierarchy(p, options={"force_rowptr64": wide})
    try:
        big = complex_rhs(n + 10, 1)
        x = big[3:3 + n]                                        # offset view (not the start of its buffer)
        ybig = complex_rhs(n + 7, 2)
        y = ybig[5:5 + n]
        y0 = y.copy()
        alpha, beta = 0.7 - 1.3j, -0.4 + 0.25j
        dev.spmv(1, mg.device.MG_OP_A, alpha, x, beta, y)
        ref = beta * y0 + alpha * (A @ x)
        assert np.abs(y - ref).max() <= 1e-13 * np.abs(ref).max()
        assert np.array_equal(ybig[:5], complex_rhs(n + 7, 2)[:5])   # nothing outside the view was written
        xr = complex_rhs(n, 4)
        bc = np.zeros(nc, dtype=np.complex128)
        dev.spmv(1, mg.device.MG_OP_R, 1.0, xr, 0.0, bc)
        refr = p.Rs[0] @ xr
        assert np.abs(bc - refr).max() <= 1e-13 * np.abs(refr).max()
        xc = complex_rhs(nc, 6)
        xf = complex_rhs(n, 8)
        xf0 = xf.copy()
        dev.spmv(1, mg.device.MG_OP_P, 1.0, xc, 1.0, xf)
        refp = xf0 + p.Ps[0] @ xc
        assert np.abs(xf - refp).max() <= 1e-13 * np.abs(refp).max()
    finally:
        dev.close()


@pytest.mark.parametrize("relax,cyc,sparse_lu", [("Jac", "V", False), ("SPAI", "W", False), ("SPAI", "F", True),
                                                 ("Jac", "W", True)])
def test_one_cycle_against_complex_oracle(mg, built, relax, cyc, sparse_lu):
    A, mesh = helmholtz(mg, [16, 16, 16], 0.5, 0.5)
    p = _param(mg, A, mesh, 3, relax, 0.8, 2, 1, cyc)
    dev = mg.device.DeviceHierarchy(p)
    try:
        if sparse_lu:                                           # the coarsest solve from the complex sparse factors
            dev._set_coarse(p, force_sparse=True)
            assert dev.lib.mg_finalize(dev.handle) == 0
        b = complex_rhs(A.shape[0], 9)
        x = np.zeros_like(b)
        dev.cycle(b, x, 1)
        xo = corc.recursiveCycle(p, b, np.zeros_like(b), 1)
        assert np.abs(x - xo).max() <= 1e-12 * np.abs(xo).max()
        # a second cycle from the first iterate (x != 0: the residual branch of MGcycle.jl:29-31)
        dev.cycle(b, x, -1)
        xo = corc.recursiveCycle(p, b, xo, 1)
        assert np.abs(x - xo).max() <= 1e-12 * np.abs(xo).max()
    finally:
        dev.close()


def test_solveMG_shifted_laplacian_64(mg, built):
    """-Lap - (1 - 0.5i) k^2 on 64^3 cells, V(2,1), SPAI, four levels.  k*h = 0.25: at k*h = 0.5 the fourth level has k*H = 4
    and the Galerkin coarse correction stops converging - in the oracle as on the device."""
    A, mesh = helmholtz(mg, [64, 64, 64], 0.25, 0.5)
    p = _param(mg, A, mesh, 4, "SPAI", 1.0, 2, 1, "V", maxIter=40, tol=1e-8)
    b = complex_rhs(A.shape[0], 12)
    x = np.zeros_like(b)
    _, _, it = mg.solveMG(p, b, x)
    hist = {}
    xo = np.zeros_like(b)
    _, ito = corc.solveMG(p, b, xo, hist)
    assert it == ito and it < 40
    assert np.abs(p.resvec - hist["resvec"]).max() <= 1e-10 * hist["resvec"][0]
    assert np.linalg.norm(b - A @ x) / np.linalg.norm(b) < p.relativeTol
    mg.clear_(p)


def test_real_operator_complex_rhs_equals_two_real_solves(mg, built):
    A, mesh = mg.poisson_shifted([32, 32, 32])
    pr = mg.getMGparam(np.float64, np.int64, 3, 8, 4, 0.0, "SPAI", 0.8, 2, 1, "V")
    pc = mg.getMGparam(np.complex128, np.int64, 3, 8, 4, 0.0, "SPAI", 0.8, 2, 1, "V")
    mg.MGsetup(A, mesh, pr)
    mg.MGsetup(A, mesh, pc)
    b = complex_rhs(A.shape[0], 13)
    x = np.zeros_like(b)
    mg.solveMG(pc, b, x)
    dev = mg.device.DeviceHierarchy(pr, options={"no_rowclass": 1})   # both through CSR
    try:
        xr = np.zeros(A.shape[0])
        xi = np.zeros(A.shape[0])
        dev.solve(np.ascontiguousarray(b.real), xr, 0.0, 4)
        dev.solve(np.ascontiguousarray(b.imag), xi, 0.0, 4)
    finally:
        dev.close()
    ref = xr + 1j * xi
    assert np.abs(x - ref).max() <= 1e-12 * np.abs(ref).max()
    mg.clear_(pc)


def test_preconditioner_for_scipy_gmres(mg, built):
    A, mesh = helmholtz(mg, [32, 32, 32], 0.5, 0.5)
    p = _param(mg, A, mesh, 3, "SPAI", 1.0, 2, 1, "V")
    b = complex_rhs(A.shape[0], 14)
    M = mg.getMultigridPreconditioner(p, b)
    n = A.shape[0]
    Mop = spla.LinearOperator((n, n), matvec=lambda v: M(np.ascontiguousarray(v, dtype=np.complex128)).copy(),
                              dtype=np.complex128)

    def run(prec):
        count = [0]
        x, info = spla.gmres(A, b, rtol=1e-8, restart=200, maxiter=3, M=prec, callback=lambda r: count.__setitem__(0, count[0] + 1),
                             callback_type="pr_norm")
        return x, info, count[0]

    x, info, its = run(Mop)
    _, _, its0 = run(None)
    assert info == 0
    assert np.linalg.norm(b - A @ x) / np.linalg.norm(b) < 1e-7
    assert its < its0
    mg.clear_(p)


def test_refusals_and_mixed_types(mg, built):
    lib = mg.device.load_library()
    vp = C.c_void_p
    h = vp()
    assert lib.mg_create_CF64(2, 2, 0, C.byref(h)) == MG_ERR_UNSUPPORTED and lib.mg_last_error()
    A, mesh = helmholtz(mg, [8, 8, 8], 0.5, 0.5)
    p = _param(mg, A, mesh, 2, "Jac", 0.8, 1, 1, "V")
    dev = mg.device.DeviceHierarchy(p)
    A8, mesh8 = mg.poisson_shifted([8, 8, 8])
    pr = mg.getMGparam(np.float64, np.int64, 2, 8, 4, 1e-10, "Jac", 0.8, 1, 1, "V")
    mg.MGsetup(A8, mesh8, pr)
    rdev = mg.device.DeviceHierarchy(pr)
    try:
        hc, hr = dev.handle, rdev.handle
        n = A.shape[0]
        bz = np.zeros(2 * n)
        xz = np.zeros(2 * n)
        dz = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        lz = C.c_longlong(0)
        lp = C.byref(lz)

        def refused(rc, code):
            assert rc == code, (rc, lib.mg_last_error())
            assert lib.mg_last_error()

        refused(lib.mg_set_cycle_type(hc, ord("K")), MG_ERR_UNSUPPORTED)
        refused(lib.mg_set_relax_type(hc, 1), MG_ERR_UNSUPPORTED)
        refused(lib.mg_set_coarse_gmres_FP64(hc, 1, dz(bz)), MG_ERR_UNSUPPORTED)
        refused(lib.mg_set_nrhs(hc, 2), MG_ERR_UNSUPPORTED)
        refused(lib.mg_cycle_CF64(hc, dz(bz), dz(xz), n, 2, 1), MG_ERR_UNSUPPORTED)
        refused(lib.mg_pcg_FP64(hc, dz(bz), dz(xz), n, 1e-6, 3, lp, lp, dz(bz)), MG_ERR_UNSUPPORTED)
        refused(lib.mg_fgmres_FP64(hc, dz(bz), dz(xz), n, 5, 1e-6, 3, lp, lp, dz(bz), lp), MG_ERR_UNSUPPORTED)
        refused(lib.mg_block_pcg_FP64(hc, dz(bz), dz(xz), n, 1, 1e-6, 3, lp, lp, dz(bz)), MG_ERR_UNSUPPORTED)
        refused(lib.mg_rap_FP64(hc, dz(bz), 1, 0, dz(bz), lp), MG_ERR_UNSUPPORTED)
        refused(lib.mg_transpose_hierarchy(hc), MG_ERR_UNSUPPORTED)
        refused(lib.mg_ghost_attach(hc, 0, 2, 1, b"\0" * 128), MG_ERR_UNSUPPORTED)
        refused(lib.mg_ghost_finalize(hc), MG_ERR_UNSUPPORTED)
        # mixed value types: FP64 entries on the CF64 handle and CF64 entries on the FP64 handle
        refused(lib.mg_cycle_FP64(hc, dz(bz), dz(xz), n, 1, 1), MG_ERR_STATE)
        refused(lib.mg_solve_FP64(hc, dz(bz), dz(xz), n, 1, 1e-6, 2, lp, dz(bz)), MG_ERR_STATE)
        refused(lib.mg_set_relax_FP64(hc, 1, dz(bz), n, 1, 1), MG_ERR_STATE)
        refused(lib.mg_set_coarse_dense_inverse_FP64(hc, 1, dz(bz)), MG_ERR_STATE)
        M = p.As[0]
        cp = np.ascontiguousarray(M.indptr, dtype=np.int64) + 1
        rv = np.ascontiguousarray(M.indices, dtype=np.int64) + 1
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_longlong))
        nzr = np.ascontiguousarray(M.data.real)
        refused(lib.mg_set_operator_FP64_INT64(hc, 1, 0, n, n, ip(cp), ip(rv), dz(nzr)), MG_ERR_STATE)
        nzc = np.ascontiguousarray(np.conj(M.data))
        refused(lib.mg_set_operator_CF64_INT64(hr, 1, 0, n, n, ip(cp), ip(rv), dz(nzc.view(np.float64))), MG_ERR_STATE)
        refused(lib.mg_cycle_CF64(hr, dz(bz), dz(xz), n, 1, 1), MG_ERR_STATE)
        refused(lib.mg_set_relax_CF64(hr, 1, dz(bz), n, 1, 1), MG_ERR_STATE)
        ab = np.zeros(2)
        refused(lib.mg_spmv_CF64(hr, 1, 0, dz(ab), dz(xz), dz(ab), dz(bz), 1), MG_ERR_STATE)
        # the Python layer: dtype mismatches and the device Krylov drivers
        with pytest.raises(TypeError):
            dev.cycle(np.zeros(n), np.zeros(n), 1)
        with pytest.raises(TypeError):
            rdev.cycle(np.zeros(A8.shape[0], dtype=np.complex128), np.zeros(A8.shape[0], dtype=np.complex128), 1)
        with pytest.raises(NotImplementedError):
            dev.pcg(np.zeros(n, dtype=np.complex128), np.zeros(n, dtype=np.complex128), 1e-6, 3)
        # the complex handle still works after all of that
        b = complex_rhs(n, 15)
        x = np.zeros_like(b)
        dev.cycle(b, x, 1)
        xo = corc.recursiveCycle(p, b, np.zeros_like(b), 1)
        assert np.abs(x - xo).max() <= 1e-12 * np.abs(xo).max()
    finally:
        dev.close()
        rdev.close()
    # a real handle created after the complex ones still matches the real oracle (tests/test_gpu_parity.py's tolerance)
    A16, mesh16 = mg.poisson_shifted([16, 16, 16])
    q = mg.getMGparam(np.float64, np.int64, 3, 8, 6, 1e-10, "Jac", 0.8, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(A16, mesh16, q)
    b = mg.seeded_rhs(A16)
    x = np.zeros_like(b)
    mg.solveMG(q, b, x)
    hist = {}
    orc.solveMG(q, b, np.zeros_like(b), False, hist)
    assert np.abs(q.resvec - hist["resvec"]).max() / hist["resvec"][0] < 1e-10
    mg.clear_(q)
