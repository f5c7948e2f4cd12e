"""-m gpu: replaceMatrixInHierarchy of ComplexF64 hierarchies on the MI355X (mg_rap_CF64, mg_get_values_CF64, mg_get_relax_CF64,
mg_replace_values_CF64, mg_replace_krylov_values_CFP64) against the host path (scipy's products, getRelaxPrec) and the complex
oracle (tests/complex_oracle.py) on the refreshed host hierarchy.

Tolerances: those of test_replace_matrix_on_device (tests/test_gpu_parity.py) and of the header of tests/test_complex_gpu.py - Galerkin
products within 1e-13 * max|entry|, relaxPrecs within 1e-13 relative, kernel-level products within 1e-13, one cycle within 1e-12,
solveMG's resvec within 1e-10 * resvec[0].  New values through the value-only paths are the same bits in HBM as a whole upload, so
the Krylov drivers must return identical arrays."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import coarse_solver_cases as cs
import complex_oracle as corc
from complex_cases import complex_rhs, helmholtz

pytestmark = pytest.mark.gpu

MG_ERR_INVALID, MG_ERR_STATE, MG_ERR_UNSUPPORTED = 1, 3, 4
DP = C.POINTER(C.c_double)


def _param(mg, A, mesh, levels, relax="SPAI", omega=1.0, pre=2, post=1, cyc="V", maxIter=8, tol=1e-10, LU=None):
    p = mg.getMGparam(np.complex128, np.int64, levels, 8, maxIter, tol, relax, omega, pre, post, cyc, "NoMUMPS", 0.5, 0.0)
    p.LU = LU
    mg.MGsetup(A, mesh, p)
    return p


def _new_matrix(A, seed):
    """The pattern of A with a seeded complex factor on every entry plus a heterogeneous complex diagonal: non-symmetric (SPAI's
    column sums differ from the row sums) and more diagonally dominant than A (the cycle keeps converging)."""
    rng = np.random.default_rng(seed)
    A2 = A.copy()
    A2.data = A.data * ((1.0 + 0.3 * rng.random(A.nnz)) + 0.2j * rng.random(A.nnz))
    dmax = np.abs(A.diagonal()).max()
    A2 = (A2 + sp.diags(dmax * (0.5 + rng.random(A.shape[0])) * (1.0 + 0.25j))).tocsr()
    A2.sort_indices()
    assert np.array_equal(A2.indptr, A.indptr) and np.array_equal(A2.indices, A.indices)
    assert np.abs((A2 - A2.T).data).max() > 0.01 * dmax
    return A2


def _assert_refreshed(mg, p, A2, relaxType, omega):
    """param.As[1:] and relaxPrecs against the host's chain of products on A2."""
    from multigrid_jl_amd.mgsetup import galerkin
    Al = A2
    for l in range(len(p.As) - 1):
        ref = mg.getRelaxPrec(Al, relaxType, omega)
        rel = np.abs(p.relaxPrecs[l] - ref) / np.abs(ref)
        Al = galerkin(p.Rs[l], Al, p.Ps[l])
        err = np.abs(Al.data - p.As[l + 1].data).max() / np.abs(Al.data).max()
        print(f"  level {l + 1}: relaxPrec rel {rel.max():.2e}, As[{l + 2}] {err:.2e} of max|entry|, longest row {np.diff(Al.indptr).max()}")
        assert p.relaxPrecs[l].dtype == np.complex128 and rel.max() <= 1e-13
        assert np.array_equal(Al.indptr, p.As[l + 1].indptr) and np.array_equal(Al.indices, p.As[l + 1].indices)
        assert err <= 1e-13


# ---- 1. the device path against the host path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("relaxType,omega,cells,chunk,groups", [("Jac", 0.8, [16, 16, 16], 0, 0), ("SPAI", 1.0, [24, 20], 0, 0),
                                                                ("Jac", 0.8, [12, 12, 12], 10, 0), ("SPAI", 1.0, [12, 12, 12], 10, 1),
                                                                ("Jac", 0.8, [24, 20], 0, 16)])
def test_replace_matrix_on_device_against_host(mg, built, monkeypatch, relaxType, omega, cells, chunk, groups):
    """chunk = 10: the 27-entry rows of the coarse operators are accumulated 10 target columns at a time.  groups: the lane groups of
    cx_rap_numeric (0: the default; 1: one row of A at a time, the walk of rap_numeric; 16: the most the option takes)."""
    if chunk:
        monkeypatch.setenv("MG_RAP_CHUNK", str(chunk))
    if groups:
        monkeypatch.setenv("MG_RAP_GROUPS", str(groups))
    A, mesh = helmholtz(mg, cells, 0.5, 0.5)
    p = _param(mg, A, mesh, 3, relaxType, omega)
    b = complex_rhs(A.shape[0], 9)
    mg.solveMG(p, b, np.zeros_like(b))                    # uploads the hierarchy
    dev_before = p.device
    assert dev_before is not None
    patterns = [(M.indptr.copy(), M.indices.copy()) for M in p.As]
    A2 = _new_matrix(A, 8)
    mg.replaceMatrixInHierarchy(p, A2)
    assert p.device is dev_before                         # stayed resident: the device path was taken
    for (ip, ix), M in zip(patterns, p.As):
        assert np.array_equal(ip, M.indptr) and np.array_equal(ix, M.indices)
    if chunk:
        assert max(np.diff(M.indptr).max() for M in p.As[1:]) > chunk
    _assert_refreshed(mg, p, A2, relaxType, omega)
    x = np.zeros_like(b)
    _, _, it = mg.solveMG(p, b, x)
    hist = {}
    _, ito = corc.solveMG(p, b, np.zeros_like(b), hist)
    diff = np.abs(p.resvec - hist["resvec"]).max() / hist["resvec"][0]
    print(f"  solveMG after the replacement: {it} cycles, resvec diff {diff:.2e}, reduction {p.resvec[-1] / p.resvec[0]:.2e}")
    assert it == ito and diff <= 1e-10
    assert p.resvec[-1] < p.resvec[0]
    # deterministic (no atomics, ordered column sums): a second pass over the same values gives the same bits
    first = [M.data.copy() for M in p.As[1:]]
    first_d = [np.array(d, copy=True) for d in p.relaxPrecs[:len(p.As) - 1]]
    mg.replaceMatrixInHierarchy(p, A2)
    assert p.device is dev_before
    for v0, M in zip(first, p.As[1:]):
        assert np.array_equal(v0, M.data)
    for d0, d in zip(first_d, p.relaxPrecs):
        assert np.array_equal(d0, d)
    mg.clear_(p)


# ---- 2. the forms of the coarsest solve ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sparse", "pjs"])
def test_replace_matrix_keeps_the_coarsest_form(mg, built, monkeypatch, form):
    """The sparse factors of the default LU (forced: no explicit inverse at any order) and a complex parallelJuliaSolver preset as
    param.LU: after the replacement the coarsest solve is the new matrix's, in the same form."""
    if form == "sparse":
        monkeypatch.setattr(mg.device, "DENSE_COARSE_MAX", 0)      # _set_coarse(p, force_sparse=True) at the upload AND at the replacement
    A, mesh = helmholtz(mg, [16, 16, 16], 0.5, 0.5)
    p = _param(mg, A, mesh, 3, "Jac", 0.8, LU=cs.pjs_lu(mg, np.complex128) if form == "pjs" else None)
    b = complex_rhs(A.shape[0], 9)
    mg.recursiveCycle(p, b, np.zeros_like(b))
    dev = p.device
    if form == "sparse":
        dev._set_coarse(p, force_sparse=True)
        assert dev.lib.mg_finalize(dev.handle) == 0
    assert dev.coarse_form()["kind"] == 1
    lu_before = p.LU
    mg.replaceMatrixInHierarchy(p, _new_matrix(A, 11))
    assert p.device is dev and dev.coarse_form()["kind"] == 1
    if form == "pjs":
        assert p.LU is lu_before                              # the solver object stays the caller's
    x = np.zeros_like(b)
    mg.recursiveCycle(p, b, x)
    q = cs.oracle_param(p, cs.SpluLU(p)) if form == "pjs" else p
    xo = corc.recursiveCycle(q, b, np.zeros_like(b), 1)
    err = np.abs(x - xo).max() / np.abs(xo).max()
    print(f"  one cycle after the replacement ({form}): {err:.2e}")
    assert err <= 1e-12
    mg.clear_(p)


# ---- 3. the C ABI on an awkward operator -----------------------------------------------------------------------------------------
def _awkward_operator(n, seed):
    """Complex square CSR with empty rows, rows spanning the kernels' 1024-entry chunks and one 3000-entry row (the operator of
    tests/test_complex_gpu.py); every row that is not empty holds its diagonal entry."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 12, n)
    lens[rng.choice(n, 40, replace=False)] = 0                 # empty rows
    lens[100:104] = [700, 650, 900, 400]
    lens[2000] = 3000
    rows, cols = [], []
    for i, k in enumerate(lens):
        c = rng.choice(n, int(k), replace=False)
        if k and i not in c:
            c[0] = i
        c = np.sort(c)
        rows.append(np.full(len(c), i))
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    A = sp.csr_matrix((np.ones(len(rows), dtype=np.complex128), (rows, cols)), shape=(n, n))
    A.sort_indices()
    return A, lens


def _values(M, seed, cplx):
    """M's pattern with seeded values."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(M.nnz) + (1j * rng.standard_normal(M.nnz) if cplx else 0.0)
    return sp.csr_matrix((v, M.indices.copy(), M.indptr.copy()), shape=M.shape)


def _manual_param(mg, A, P, R, Ac, d):
    """A two-level complex param around arbitrary operators; the coarsest solve is a well-conditioned matrix of its own (a two-level
    cycle never applies As[2], it only solves with param.LU)."""
    nc = P.shape[1]
    p = mg.getMGparam(np.complex128, np.int64, 2, 8, 4, 1e-10, "Jac", 0.8, 1, 1, "V")
    p.As, p.Ps, p.Rs = [A, Ac], [P], [R]
    p.relaxPrecs = [d]
    S = (sp.identity(nc) * (4.0 + 1j) + 0.1 * sp.random(nc, nc, density=0.05, random_state=5)).tocsc().astype(np.complex128)
    p.LU = spla.splu(S)
    p.nrhs = 1
    return p


def test_c_abi_on_an_awkward_operator(mg, built):
    n, nc = 5000, 700
    D = mg.device
    pat, lens = _awkward_operator(n, 3)
    P0 = sp.random(n, nc, density=4.0 / nc, random_state=7, format="csr")
    R0 = sp.random(nc, n, density=6.0 / n, random_state=8, format="csr")
    P0.sort_indices()
    R0.sort_indices()
    assert (np.diff(P0.indptr) == 0).any() and (np.diff(R0.indptr) == 0).any()       # empty rows in P and R too
    A0 = _values(pat, 1, True)
    Cpat = (abs(R0) @ (abs(pat) @ abs(P0))).tocsr()                                # the structural product
    Cpat.sort_indices()
    assert (np.diff(Cpat.indptr) == 0).any() and np.diff(Cpat.indptr).max() > 5 * 64   # empty rows; rows of many passes of 64
    rng = np.random.default_rng(2)
    d0 = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    p = _manual_param(mg, A0, P0, R0, _values(Cpat, 4, True), d0)
    lib = D.load_library()
    dev = D.DeviceHierarchy(p, options={"rap_chunk": 64})
    wide = None
    A8, mesh8 = mg.poisson_shifted([8, 8, 8])
    pr = mg.getMGparam(np.float64, np.int64, 2, 8, 4, 1e-10, "Jac", 0.8, 1, 1, "V")
    mg.MGsetup(A8, mesh8, pr)
    rdev = D.DeviceHierarchy(pr)
    try:
        h = dev.handle
        done = C.c_longlong(0)
        ptr = lambda a: a.ctypes.data_as(DP)
        at = lambda M: np.ascontiguousarray(np.conj(M.data), dtype=np.complex128)    # the reference's AT values
        # -- mg_rap_CF64 + mg_get_values_CF64 + mg_get_relax_CF64, both kinds
        A1 = _values(pat, 11, True)
        ref = (R0 @ (A1 @ P0)).tocsr()
        ref.sort_indices()
        assert np.array_equal(ref.indptr, Cpat.indptr) and np.array_equal(ref.indices, Cpat.indices)
        om = np.array([0.8, 0.0])
        ms = np.zeros(1)
        assert lib.mg_rap_level_ms_CF64(h, ptr(ms), 1) == MG_ERR_STATE and lib.mg_last_error()      # no re-setup yet
        for kind, name in ((0, "Jac"), (1, "SPAI")):
            nz = at(A1)
            assert lib.mg_rap_CF64(h, ptr(nz), nz.size, kind, ptr(om), C.byref(done)) == 0, lib.mg_last_error()
            assert done.value == 1
            got = dev.get_values(2, D.MG_OP_A)
            err = np.abs(got - ref.data).max() / np.abs(ref.data).max()
            assert np.array_equal(dev.get_values(1, D.MG_OP_A), A1.data)          # the fine values: conjugated in, conjugated out
            dgot = np.zeros(n, dtype=np.complex128)
            assert lib.mg_get_relax_CF64(h, 1, ptr(dgot), n) == 0, lib.mg_last_error()
            with np.errstate(all="ignore"):
                dref = mg.getRelaxPrec(A1, name, 0.8)
            ok = np.isfinite(dref)
            assert np.array_equal(ok, np.isfinite(dgot)) and ok.sum() >= n - 40 and (kind == 1 or ok.sum() == n - 40)
            rel = (np.abs(dgot[ok] - dref[ok]) / np.maximum(np.abs(dref[ok]), 1e-300)).max()
            print(f"  {name}: As[2] {err:.2e} of max|entry|, relaxPrec rel {rel:.2e}")
            assert err <= 1e-13 and rel <= 1e-13
        # -- the device time of the last re-setup, one value per level below the coarsest
        assert lib.mg_rap_level_ms_CF64(h, ptr(ms), 1) == 0, lib.mg_last_error()
        assert 0.0 < ms[0] < 1e4 and np.array_equal(dev.rap_level_ms(), ms)
        assert lib.mg_rap_level_ms_CF64(h, ptr(ms), 2) == MG_ERR_INVALID and lib.mg_last_error()
        assert lib.mg_rap_level_ms_CF64(h, None, 1) == MG_ERR_INVALID
        assert lib.mg_rap_level_ms_CF64(rdev.handle, ptr(ms), 1) == MG_ERR_STATE
        # -- the default options: rows of 700 target columns in one pass, the lane groups cut down to what fits the LDS
        dflt = D.DeviceHierarchy(p)
        try:
            nz = at(A1)
            assert lib.mg_rap_CF64(dflt.handle, ptr(nz), nz.size, 0, ptr(om), None) == 0, lib.mg_last_error()
            err = np.abs(dflt.get_values(2, D.MG_OP_A) - ref.data).max() / np.abs(ref.data).max()
            print(f"  default options: As[2] {err:.2e} of max|entry|")
            assert err <= 1e-13
        finally:
            dflt.close()
        # -- mg_replace_values_CF64 + mg_spmv_CF64 for A, P and R
        A2, P2, R2 = _values(pat, 12, True), _values(P0, 13, False), _values(R0, 14, False)
        dev.replace_values(1, D.MG_OP_A, A2)
        dev.replace_values(1, D.MG_OP_P, P2)
        dev.replace_values(1, D.MG_OP_R, R2)
        assert np.array_equal(dev.get_values(1, D.MG_OP_P), P2.data) and np.array_equal(dev.get_values(1, D.MG_OP_R), R2.data)
        for which, M in ((D.MG_OP_A, A2), (D.MG_OP_P, P2), (D.MG_OP_R, R2)):
            x = complex_rhs(M.shape[1], 20 + which)
            y = np.zeros(M.shape[0], dtype=np.complex128)
            dev.spmv(1, which, 1.0, x, 0.0, y)
            want = M @ x
            assert np.abs(y - want).max() <= 1e-13 * np.abs(want).max()
        # -- refusals: the code and a message, nothing changed
        def refused(rc, code):
            assert rc == code, (rc, lib.mg_last_error())
            assert lib.mg_last_error()

        nz = at(A1)
        refused(lib.mg_rap_CF64(None, ptr(nz), nz.size, 0, ptr(om), None), MG_ERR_INVALID)
        refused(lib.mg_rap_CF64(h, None, nz.size, 0, ptr(om), None), MG_ERR_INVALID)
        refused(lib.mg_rap_CF64(h, ptr(nz), nz.size, 0, None, None), MG_ERR_INVALID)
        refused(lib.mg_rap_CF64(h, ptr(nz), nz.size - 1, 0, ptr(om), None), MG_ERR_INVALID)
        refused(lib.mg_rap_CF64(h, ptr(nz), nz.size, 2, ptr(om), None), MG_ERR_INVALID)
        rz = np.zeros(2 * A8.nnz)
        refused(lib.mg_rap_CF64(rdev.handle, ptr(rz), A8.nnz, 0, ptr(om), None), MG_ERR_STATE)
        refused(lib.mg_get_values_CF64(rdev.handle, 1, 0, ptr(rz), A8.nnz), MG_ERR_STATE)
        refused(lib.mg_get_relax_CF64(rdev.handle, 1, ptr(rz), A8.shape[0]), MG_ERR_STATE)
        refused(lib.mg_replace_values_CF64(rdev.handle, 1, 0, ptr(rz), A8.nnz), MG_ERR_STATE)
        refused(lib.mg_replace_krylov_values_CFP64(rdev.handle, ptr(rz), A8.nnz), MG_ERR_STATE)
        refused(lib.mg_get_values_CF64(h, 1, 0, ptr(nz), nz.size + 1), MG_ERR_INVALID)
        refused(lib.mg_get_values_CF64(h, 1, 0, None, nz.size), MG_ERR_INVALID)
        refused(lib.mg_get_values_CF64(h, 2, D.MG_OP_P, ptr(nz), 1), MG_ERR_INVALID)      # the coarsest level has no transfer operators
        refused(lib.mg_get_relax_CF64(h, 1, ptr(nz), n + 1), MG_ERR_INVALID)
        refused(lib.mg_replace_values_CF64(h, 1, D.MG_OP_P, ptr(nz), P0.nnz + 1), MG_ERR_INVALID)
        refused(lib.mg_replace_values_CF64(h, 1, 7, ptr(nz), nz.size), MG_ERR_INVALID)
        refused(lib.mg_replace_krylov_values_CFP64(h, ptr(nz), nz.size), MG_ERR_STATE)    # no Krylov operator set
        dev.set_krylov_operator(A2)
        refused(lib.mg_replace_krylov_values_CFP64(h, ptr(nz), nz.size - 1), MG_ERR_INVALID)
        refused(lib.mg_replace_krylov_values_CFP64(h, None, nz.size), MG_ERR_INVALID)
        dev.set_krylov_operator(None)
        wide = D.DeviceHierarchy(p, options={"force_rowptr64": 1})
        refused(lib.mg_rap_CF64(wide.handle, ptr(nz), nz.size, 0, ptr(om), None), MG_ERR_UNSUPPORTED)
        # a handle that is not finalized (a relaxPrec was set since): refused, then finalized again with finite relaxPrecs
        dev._set_relax(1, d0, 1, 1)
        refused(lib.mg_rap_CF64(h, ptr(nz), nz.size, 0, ptr(om), None), MG_ERR_STATE)
        assert lib.mg_finalize(h) == 0
        # -- the handle still cycles, with the values written last
        assert np.array_equal(dev.get_values(1, D.MG_OP_A), A2.data)
        p.As[0], p.Ps[0], p.Rs[0] = A2, P2, R2
        b = complex_rhs(n, 15)
        x = np.zeros_like(b)
        dev.cycle(b, x, 1)
        xo = corc.recursiveCycle(p, b, np.zeros_like(b), 1)
        assert np.abs(x - xo).max() <= 1e-12 * np.abs(xo).max()
    finally:
        dev.close()
        rdev.close()
        if wide is not None:
            wide.close()


# ---- 4. the Krylov operator ------------------------------------------------------------------------------------------------------
def test_update_krylov_operator(mg, built):
    """New values on the pattern uploaded last replace the resident ones (no upload of the pattern); the drivers then return the
    arrays of a fresh handle that uploaded the new operator whole."""
    Ah, mesh = helmholtz(mg, [8, 8, 8], 0.5, 0.5)
    p = _param(mg, Ah, mesh, 2, "SPAI", 1.0)
    As, _ = helmholtz(mg, [8, 8, 8], 0.5, 0.05)
    rng = np.random.default_rng(31)
    A_new = As.copy()
    A_new.data = As.data * (1.0 + 0.1 * rng.random(As.nnz))
    A_other = (A_new + sp.csr_matrix(([0.5 - 0.25j], ([3], [As.shape[0] - 4])), shape=As.shape)).tocsr()   # one entry more
    assert A_other.nnz == A_new.nnz + 1
    b = complex_rhs(As.shape[0], 21)

    def run(dev):
        x1, x2 = np.zeros_like(b), np.zeros_like(b)
        _, f1, i1, r1 = dev.bicgstab(b, x1, 1e-8, 40)
        _, f2, i2, r2 = dev.fgmres(b, x2, 5, 1e-8, 20)
        assert f1 in (0, -3) and f2 == 0
        return (x1, i1, r1.copy()), (x2, i2, r2.copy())

    def same(got, want):
        for (xg, ig, rg), (xw, iw, rw) in zip(got, want):
            assert ig == iw and np.array_equal(rg, rw) and np.array_equal(xg, xw)

    dev, fresh = mg.device.DeviceHierarchy(p), mg.device.DeviceHierarchy(p)
    try:
        dev.set_krylov_operator(As)
        before = run(dev)
        pat = dev._krylov_pattern
        dev.update_krylov_operator(A_new)                       # the same pattern: values only
        assert dev.krylov_operator is A_new and dev._krylov_pattern is pat
        fresh.set_krylov_operator(A_new)
        want = run(fresh)
        got = run(dev)
        same(got, want)
        assert not np.array_equal(got[0][2], before[0][2])      # (the values did change)
        dev.update_krylov_operator(A_other)                     # another pattern: the whole upload
        assert dev.krylov_operator is A_other and dev._krylov_pattern is not pat and dev._krylov_pattern[2].size == A_other.nnz
        fresh.set_krylov_operator(A_other)
        same(run(dev), run(fresh))
        with pytest.raises(mg.device.MGDeviceError):            # a wrong order: refused, the previous object stays
            dev.update_krylov_operator(sp.identity(As.shape[0] - 1, dtype=np.complex128, format="csr"))
        assert dev.krylov_operator is A_other
        same(run(dev), run(fresh))                              # ... and so does its operator in HBM
    finally:
        dev.close()
        fresh.close()


# ---- 5. the loop a user writes ---------------------------------------------------------------------------------------------------
def test_inversion_loop_keeps_the_hierarchy_resident(mg, built):
    """Two successive media on one grid: the hierarchy on the damped operator is refreshed in HBM (replaceMatrixInHierarchy), the
    undamped Krylov operator gets new values, BiCGSTAB solves each system."""
    cells, kh = [16, 16, 16], 0.5
    mesh = mg.getRegularMesh([0.0, 1.0] * 3, cells)
    L = mg.getNodalLaplacianMatrix(mesh).tocsr().astype(np.complex128)
    n = L.shape[0]
    k2 = kh * kh * L.diagonal().real.max() / 6.0

    def operator(m, damping):
        A = (L - sp.diags((1.0 - damping * 1j) * k2 * m, format="csr")).tocsr()
        A.sort_indices()
        return A

    rng = np.random.default_rng(41)
    media = [np.ones(n)] + [0.7 + 0.3 * rng.random(n) for _ in range(2)]
    p = mg.getMGparam(np.complex128, np.int64, 3, 8, 60, 1e-8, "SPAI", 1.0, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(operator(media[0], 0.5), mesh, p)
    b = complex_rhs(n, 21)
    mg.solveBiCGSTAB_MG_CFP64(operator(media[0], 0.05), p, b, np.zeros_like(b))       # uploads the hierarchy and the operator
    dev = p.device
    pat = dev._krylov_pattern
    assert dev is not None and pat is not None
    for m in media[1:]:
        mg.replaceMatrixInHierarchy(p, operator(m, 0.5))
        A_sys = operator(m, 0.05)
        x = np.zeros_like(b)
        _, _, it, _ = mg.solveBiCGSTAB_MG_CFP64(A_sys, p, b, x)
        res = np.linalg.norm(b - A_sys @ x) / np.linalg.norm(b)
        print(f"  medium: {it} iterations, flag {p.flag}, ||b - A x|| / ||b|| = {res:.2e}")
        assert p.device is dev and dev.krylov_operator is A_sys and dev._krylov_pattern is pat
        assert res < 1e-6
    mg.clear_(p)
