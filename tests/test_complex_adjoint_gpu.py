"""-m gpu: adjointHierarchy of complex hierarchies on the MI355X (mg_adjoint_hierarchy_CF64 / _CF32: the cx_adj_* kernels of
csrc/mg_complex.hpp) against the host mirror (scipy's conjugate transposes), the complex oracles on the flipped host hierarchy and,
for ComplexF32, a fresh upload of the host-flipped param.

Tolerances are the project's own (tests/test_complex_gpu.py): kernel-level products within 1e-13, one cycle within 1e-12, solveMG's
resvec within 1e-10 * resvec[0]; K-cycle / Jac-GMRES / GMRES-coarsest cycles within 1e-11 with the clearances their oracles ask for
(tests/test_complex_kcycle_gpu.py, tests/test_complex_coarse_gmres_gpu.py); ComplexF32 cycles 64 * 2^-24 in the rel2 measure.  Operators,
relaxPrecs and the GMRES coarsest vector are permutations and sign flips of what was uploaded: those are compared bit for bit."""
import copy
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import coarse_solver_cases as csc
import complex_coarse_cases as cc
import complex_kcycle_oracle as korc
import complex_oracle as corc
import complex_single_oracle as cs
from complex_adjoint_cases import adjoint_sorted, base_operator, base_param, oracle_param, same_csr
from complex_cases import complex_rhs, helmholtz

pytestmark = pytest.mark.gpu

MG_OK, MG_ERR_STATE, MG_ERR_UNSUPPORTED = 0, 3, 4
U32 = 2.0 ** -24
_dp = C.POINTER(C.c_double)


def _assert_device_holds(mg, dev, p):
    """Every A, P, R and relaxPrecs in HBM equal the host mirror's arrays, bit for bit."""
    D = mg.device
    nl = len(p.As)
    for l in range(1, nl + 1):
        assert np.array_equal(dev.get_values(l, D.MG_OP_A), p.As[l - 1].data), f"As[{l}]"
        if l < nl:
            assert np.array_equal(dev.get_values(l, D.MG_OP_P), p.Ps[l - 1].data), f"Ps[{l}]"
            assert np.array_equal(dev.get_values(l, D.MG_OP_R), p.Rs[l - 1].data), f"Rs[{l}]"
            d = np.empty(p.As[l - 1].shape[0], dtype=np.complex128)
            assert dev.lib.mg_get_relax_CF64(dev.handle, l, d.ctypes.data_as(_dp), d.size) == MG_OK
            assert np.array_equal(d, p.relaxPrecs[l - 1]), f"relaxPrecs[{l}]"


def _oracle_solve(p, b):
    """(x, resvec) of tests/complex_oracle.py's solveMG on p; with the GMRES coarsest solve its breaks must be clear of 0.01."""
    q = oracle_param(p)
    hist = {}
    xo = np.zeros_like(b)
    corc.solveMG(q, b, xo, hist)
    if p.coarseSolveType == "GMRES":
        assert cc.clearance(q.LU.log) >= cc.MIN_CLEARANCE, cc.clearance(q.LU.log)
    return xo, hist["resvec"]


def _solve_matches_oracle(mg, p, b, what):
    x = np.zeros_like(b)
    mg.solveMG(p, b, x)
    xo, rvo = _oracle_solve(p, b)
    dr = np.abs(p.resvec - rvo).max() / rvo[0]
    dx = np.abs(x - xo).max() / np.abs(xo).max()
    true = np.linalg.norm(p.As[0] @ x - b)
    print(f"  {what}: resvec {dr:.2e}, x {dx:.2e}, |true residual - resvec[-1]| / resvec[0] = {abs(true - p.resvec[-1]) / p.resvec[0]:.2e}")
    assert len(p.resvec) == len(rvo) and dr <= 1e-10 and dx <= 1e-10
    return x


# ---- 1. the base case, ComplexF64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relax,coarse", [("Jac", "NoMUMPS"), ("SPAI", "NoMUMPS"), ("Jac", "GMRES"), ("SPAI", "GMRES")])
def test_adjoint_on_the_resident_hierarchy(mg, built, relax, coarse):
    """Fails without the feature on a GPU machine: AttributeError."""
    p, A, _ = base_param(mg, relax, coarse)
    b = complex_rhs(A.shape[0], 9)
    try:
        _solve_matches_oracle(mg, p, b, f"{relax} {coarse} forward")
        dev = p.device
        assert dev is not None
        As0 = [M.copy() for M in p.As]
        mg.adjointHierarchy(p)
        assert p.device is dev and p.doTranspose == 1                   # flipped in HBM, not dropped
        assert dev.coarse_form()["kind"] == (3 if coarse == "GMRES" else 0)
        _assert_device_holds(mg, dev, p)
        x = _solve_matches_oracle(mg, p, b, f"{relax} {coarse} adjoint")
        true = np.linalg.norm(A.conj().T @ x - b)
        assert abs(true - p.resvec[-1]) <= 1e-8 * p.resvec[0]           # (it is A' x = b that was solved)
        mg.adjointHierarchy(p)
        assert p.device is dev and p.doTranspose == 0
        for M, M0 in zip(p.As, As0):
            assert same_csr(M, M0)
        _assert_device_holds(mg, dev, p)
        x = _solve_matches_oracle(mg, p, b, f"{relax} {coarse} flipped twice")
        assert abs(np.linalg.norm(A @ x - b) - p.resvec[-1]) <= 1e-8 * p.resvec[0]
    finally:
        mg.clear_(p)


def test_the_same_bits_on_every_run(mg, built):
    """Two handles flipped from the same upload hold the same arrays (the scatter's order does not reach the result)."""
    p, A, _ = base_param(mg, "SPAI")
    devs = [mg.device.DeviceHierarchy(p) for _ in range(2)]
    try:
        for dev in devs:
            assert dev.lib.mg_adjoint_hierarchy_CF64(dev.handle) == MG_OK
        mg.adjointHierarchy(p)                                          # (no resident hierarchy: the host mirror alone)
        for dev in devs:
            _assert_device_holds(mg, dev, p)
        b = complex_rhs(A.shape[0], 9)
        xs = [dev.cycle(b, np.zeros_like(b), 1).copy() for dev in devs]
        assert np.array_equal(xs[0], xs[1])
        for dev in devs:                                                # the _CF32 entry refuses a CF64 handle and changes nothing
            assert dev.lib.mg_adjoint_hierarchy_CF32(dev.handle) == MG_ERR_STATE
        assert np.array_equal(devs[0].cycle(b, np.zeros_like(b), 1), xs[0])
    finally:
        for dev in devs:
            dev.close()


# ---- 2. ComplexF32 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relax", ["Jac", "SPAI"])
def test_single_precision_flip_equals_a_fresh_upload(mg, built, relax):
    """get_values is not served for CF32 handles: one cycle of the resident hierarchy flipped in HBM equals, bit for bit, one cycle of
    a fresh upload of the host-flipped param (GMRES coarsest solve: operators, relaxPrecs and d are permutations and sign flips, the
    widened coarsest operator is rebuilt from the same single values)."""
    p, A, _ = base_param(mg, relax, "GMRES", single=True)
    b = complex_rhs(A.shape[0], 9).astype(np.complex64)
    fresh = None
    try:
        mg.recursiveCycle(p, b, np.zeros_like(b))
        dev = p.device
        assert dev is not None and dev.coarse_form()["kind"] == 3
        assert dev.lib.mg_adjoint_hierarchy_CF64(dev.handle) == MG_ERR_STATE      # the _CF64 entry refuses a CF32 handle
        for flip in (1, 2):
            mg.adjointHierarchy(p)
            assert p.device is dev and p.doTranspose == flip % 2
            x = np.zeros_like(b)
            dev.cycle(b, x, 1)
            fresh = mg.device.DeviceHierarchy(p)
            xf = np.zeros_like(b)
            fresh.cycle(b, xf, 1)
            fresh.close()
            fresh = None
            assert np.array_equal(x, xf), f"flip {flip}: {cs.rel2(x, xf):.3e}"
            q = cc.oracle_param(p)
            xo = cs.recursiveCycle(q, b, np.zeros_like(b), 1).copy()
            assert cc.clearance(q.LU.log) >= cc.MIN_CLEARANCE
            e = cs.rel2(x, xo)
            print(f"  ComplexF32 {relax} flip {flip}: rel2 {e:.2e} from the single oracle (bound {64 * U32:.2e})")
            assert e < 64 * U32
    finally:
        if fresh is not None:
            fresh.close()
        mg.clear_(p)


def test_single_precision_driver_after_the_flip(mg, built):
    """The ComplexF64 BiCGSTAB on a flipped CF32 handle (dense coarsest inverse, ComplexF64, flipped in place): the Krylov operator
    widened from As[1] before the flip must be widened again from the new As[1], or the driver would solve A x = b."""
    p, A, _ = base_param(mg, "SPAI", single=True, maxIter=100, tol=1e-6)
    b = complex_rhs(A.shape[0], 9)
    try:
        x = np.zeros_like(b)
        mg.solveBiCGSTAB_MG_CFP64(p.As[0], p, b, x)
        assert p.flag in (0, -3)                                       # (-3: converged at the half step)
        dev = p.device
        Af = p.As[0].astype(np.complex128)
        assert np.linalg.norm(Af @ x - b) <= 1e-5 * np.linalg.norm(b)
        mg.adjointHierarchy(p)
        assert p.device is dev
        x = np.zeros_like(b)
        _, _, it, _ = mg.solveBiCGSTAB_MG_CFP64(p.As[0], p, b, x)
        res = np.linalg.norm(Af.conj().T @ x - b) / np.linalg.norm(b)
        print(f"  ComplexF32 BiCGSTAB on A': {it} iterations, flag {p.flag}, true residual {res:.2e}")
        assert p.flag == 0 and res <= 1e-5
    finally:
        mg.clear_(p)


# ---- 3. kernel corners -----------------------------------------------------------------------------------------------------------
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


def _products_match_scipy(mg, dev, p, n, nc):
    D = mg.device
    x = complex_rhs(n, 4)
    y = np.zeros(n, dtype=np.complex128)
    dev.spmv(1, D.MG_OP_A, 1.0, x, 0.0, y)
    ref = p.As[0] @ x
    ea = np.abs(y - ref).max() / np.abs(ref).max()
    xc = complex_rhs(nc, 6)
    xf = complex_rhs(n, 8)
    refp = xf + p.Ps[0] @ xc
    dev.spmv(1, D.MG_OP_P, 1.0, xc, 1.0, xf)
    ep = np.abs(xf - refp).max() / np.abs(refp).max()
    bc = np.zeros(nc, dtype=np.complex128)
    dev.spmv(1, D.MG_OP_R, 1.0, x, 0.0, bc)
    refr = p.Rs[0] @ x
    er = np.abs(bc - refr).max() / np.abs(refr).max()
    print(f"  products: A {ea:.2e}, P {ep:.2e}, R {er:.2e}")
    assert ea <= 1e-13 and ep <= 1e-13 and er <= 1e-13


def test_adjoint_of_an_awkward_operator(mg, built):
    """Empty rows and columns, rows of 400 to 900 entries and one of 3000: after the first adjoint they are long COLUMNS of the
    source; after the second the 3000-entry row is an OUTPUT row longer than a chunk - the one-long-row branch of the rebuilt block
    table.  P <- R' is 5000 x 700 with empty rows."""
    n, nc = 5000, 700
    A = _awkward_operator(n, 3)
    p = _manual_param(mg, A, nc, 7)
    R0 = p.Rs[0].copy()
    assert (np.diff(A.indptr) == 0).any() and (np.diff(adjoint_sorted(A).indptr) == 0).any()
    dev = p.device = mg.device.DeviceHierarchy(p)
    try:
        mg.adjointHierarchy(p)
        assert p.device is dev
        assert same_csr(p.As[0], adjoint_sorted(A)) and p.Ps[0].shape == (n, nc) and same_csr(p.Ps[0], adjoint_sorted(R0))
        assert np.diff(p.As[0].indptr).max() < 1024 and (np.diff(p.Ps[0].indptr) == 0).any()
        _assert_device_holds(mg, dev, p)
        _products_match_scipy(mg, dev, p, n, nc)
        mg.adjointHierarchy(p)
        assert p.device is dev and same_csr(p.As[0], A) and np.diff(p.As[0].indptr).max() == 3000
        _assert_device_holds(mg, dev, p)
        _products_match_scipy(mg, dev, p, n, nc)
    finally:
        mg.clear_(p)


# ---- 4. refusals leave the handle as it was ----------------------------------------------------------------------------------------
def _long_column_param(mg):
    """6000 rows, column 0 with 5000 entries (beyond the 4096 the per-column ranking takes), a dominant complex diagonal."""
    n, nc = 6000, 700
    col = sp.csr_matrix((np.full(4999, 0.01 + 0.02j), (np.arange(1, 5000), np.zeros(4999, dtype=int))), shape=(n, n))
    A = (sp.identity(n, dtype=np.complex128) * (4.0 + 1.0j) + sp.diags([np.linspace(0.1, 0.4, n - 1)], [1]) * (1.0 + 0.3j) + col).tocsr()
    A.sort_indices()
    assert np.bincount(A.indices, minlength=n).max() == 5000
    p = _manual_param(mg, A, nc, 11)
    p.relaxPrecs = [np.ascontiguousarray(0.8 / A.diagonal())]
    return p


def _refusal_case(mg, name):
    """(param with its resident hierarchy in param.device, right-hand side)"""
    if name == "schwarz":
        A, mesh = helmholtz(mg, [32, 32], 0.5, 0.5)
        p = csc.setup(mg, A, mesh, 3, csc.dd_lu(mg, mesh, [2, 2], [1, 1], np.complex128), np.complex128, "Jac", 0.8, 2, 2, "V", 12, 1e-8)
        b = complex_rhs(A.shape[0], 9)
        mg.recursiveCycle(p, b, np.zeros_like(b))
        assert p.device.coarse_form()["kind"] == 4                    # a Schwarz sweep
        return p, b
    if name == "long_column":
        p = _long_column_param(mg)
        p.device = mg.device.DeviceHierarchy(p)
        return p, complex_rhs(6000, 9)
    p, A, _ = base_param(mg, "SPAI")
    options = {"rowptr64": {"force_rowptr64": 1}, "sparse_factors_chip_wide": {"lu_multi_min_rows": 0}}.get(name)
    p.device = mg.device.DeviceHierarchy(p, options=options)
    if name.startswith("sparse_factors"):
        p.device._set_coarse(p, force_sparse=True)
        assert p.device.lib.mg_finalize(p.device.handle) == MG_OK
        assert p.device.coarse_form()["kind"] == (2 if name.endswith("chip_wide") else 1)
    return p, complex_rhs(A.shape[0], 9)


@pytest.mark.parametrize("name", ["rowptr64", "long_column", "sparse_factors", "sparse_factors_chip_wide", "schwarz"])
def test_refusals_leave_the_handle_as_it_was(mg, built, name):
    p, b = _refusal_case(mg, name)
    try:
        dev = p.device
        before = dev.cycle(b, np.zeros_like(b), 1).copy()
        assert dev.lib.mg_adjoint_hierarchy_CF64(dev.handle) == MG_ERR_UNSUPPORTED
        assert dev.lib.mg_last_error()
        assert np.array_equal(dev.cycle(b, np.zeros_like(b), 1), before)   # the old bits
        A0 = p.As[0].copy()
        mg.adjointHierarchy(p)                                              # the host falls back: released, uploaded again lazily
        assert p.device is None and p.doTranspose == 1 and same_csr(p.As[0], adjoint_sorted(A0))
        x = np.zeros_like(b)
        mg.recursiveCycle(p, b, x)
        assert p.device is not None and p.device is not dev
        xo = corc.recursiveCycle(p, b, np.zeros_like(b), 1)
        e = np.abs(x - xo).max() / np.abs(xo).max()
        print(f"  {name}: one cycle of the re-uploaded adjoint hierarchy {e:.2e} from the oracle")
        assert e <= 1e-12
    finally:
        mg.clear_(p)


# ---- 5. schedules --------------------------------------------------------------------------------------------------------------------
_SCHEDULES = {"K-Jac": ("Jac", "K", "NoMUMPS"), "V-JacGMRES-coarseGMRES": ("Jac-GMRES", "V", "GMRES")}


def _schedule_param(mg, name):
    relax, cyc, coarse = _SCHEDULES[name]
    A, mesh = base_operator(mg, (16, 16, 16))
    p = mg.getMGparam(np.complex128, np.int64, 3, 8, 5, 1e-10, relax, 0.8, 2, 1, cyc, coarse, 0.5, 0.0)
    mg.MGsetup(A, mesh, p)
    return p, complex_rhs(A.shape[0], 9)


def _schedule_oracle(p, b):
    """One cycle of tests/complex_kcycle_oracle.py on p from zero; its discrete decisions must be clear of their thresholds."""
    q = oracle_param(p)
    trace = []
    xo = korc.recursiveCycle(q, b, np.zeros_like(b), 1, trace=trace).copy()
    assert len(trace) > 0 and korc.rn_clear_of_tol(trace, 4.0), korc.all_rn(trace)
    if p.coarseSolveType == "GMRES":
        assert cc.clearance(q.LU.log) >= cc.MIN_CLEARANCE, cc.clearance(q.LU.log)
    return xo


@pytest.mark.parametrize("name", list(_SCHEDULES))
def test_schedules_after_the_flip(mg, built, name):
    p, b = _schedule_param(mg, name)
    try:
        x = np.zeros_like(b)
        mg.recursiveCycle(p, b, x)
        dev = p.device
        e0 = np.abs(x - _schedule_oracle(p, b)).max() / np.abs(x).max()
        mg.adjointHierarchy(p)
        assert p.device is dev
        _assert_device_holds(mg, dev, p)
        xo = _schedule_oracle(p, b)
        x = np.zeros_like(b)
        mg.recursiveCycle(p, b, x)
        e1 = np.abs(x - xo).max() / np.abs(xo).max()
        print(f"  {name}: one cycle forward {e0:.2e}, after the flip {e1:.2e}")
        assert e0 <= 1e-11 and e1 <= 1e-11
    finally:
        mg.clear_(p)


# ---- 6. re-setup after a flip ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relax,omega", [("Jac", 0.8), ("SPAI", 0.8)])
def test_replace_matrix_after_a_flip(mg, built, relax, omega):
    """replaceMatrixInHierarchy with a matrix on the pattern NOW held stays on the device and sets doTranspose back to 0; values and
    relaxPrecs equal the host path on a twin of the flipped param (the comparison of tests/test_complex_rap_gpu.py).  SPAI: the column
    sums come from the transposed pattern, which is the one of the flipped operator only if the stale one was dropped."""
    p, A, _ = base_param(mg, relax)
    b = complex_rhs(A.shape[0], 9)
    try:
        if relax == "SPAI":                                       # a re-setup BEFORE the flip caches the transposed pattern of As[l]
            mg.recursiveCycle(p, b, np.zeros_like(b))
            mg.replaceMatrixInHierarchy(p, A)
        mg.recursiveCycle(p, b, np.zeros_like(b))
        dev = p.device
        mg.adjointHierarchy(p)
        assert p.device is dev and p.doTranspose == 1
        rng = np.random.default_rng(8)
        At = p.As[0]
        A2 = At.copy()
        A2.data = At.data * ((1.0 + 0.3 * rng.random(At.nnz)) + 0.2j * rng.random(At.nnz))
        A2 = (A2 + sp.diags(np.abs(At.diagonal()).max() * (0.5 + rng.random(At.shape[0])) * (1.0 + 0.25j))).tocsr()
        A2.sort_indices()
        assert np.array_equal(A2.indptr, At.indptr) and np.array_equal(A2.indices, At.indices)
        twin = copy.copy(p)
        twin.device, twin.LU = None, None
        twin.As, twin.Ps, twin.Rs = [M.copy() for M in p.As], list(p.Ps), list(p.Rs)
        twin.relaxPrecs = [np.array(d, copy=True) for d in p.relaxPrecs]
        mg.replaceMatrixInHierarchy(twin, A2)
        mg.replaceMatrixInHierarchy(p, A2)
        assert p.device is dev and p.doTranspose == 0
        for l in range(len(p.As)):
            assert np.array_equal(p.As[l].indptr, twin.As[l].indptr) and np.array_equal(p.As[l].indices, twin.As[l].indices)
            err = np.abs(p.As[l].data - twin.As[l].data).max() / np.abs(twin.As[l].data).max()
            assert err <= 1e-13, (l, err)
        for l in range(len(p.As) - 1):
            rel = (np.abs(p.relaxPrecs[l] - twin.relaxPrecs[l]) / np.abs(twin.relaxPrecs[l])).max()
            assert rel <= 1e-13, (l, rel)
        _assert_device_holds(mg, dev, p)
        x = np.zeros_like(b)
        mg.recursiveCycle(p, b, x)
        xo = corc.recursiveCycle(p, b, np.zeros_like(b), 1)
        assert np.abs(x - xo).max() <= 1e-12 * np.abs(xo).max()
    finally:
        mg.clear_(p)


# ---- 7. end to end -------------------------------------------------------------------------------------------------------------------
def test_solve_linear_system_flips_one_resident_handle(mg, built):
    """Fails without the feature on a GPU machine (NotImplementedError from transposeHierarchy).  A complex MGsolver("BiCGSTAB",
    sym = 0) solving A x = b, A' x = b, A x = b: one upload, two flips in HBM, every solve to tol on its own system."""
    A, mesh = base_operator(mg)
    p = mg.getMGparam(np.complex128, np.int64, 3, 8, 100, 1e-6, "SPAI", 0.8, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
    s = mg.getMGsolver(p, mesh, 0, "BiCGSTAB")
    b = complex_rhs(A.shape[0], 9)
    dev = None
    try:
        for k, t in enumerate((0, 1, 0)):
            x = np.zeros_like(b)
            mg.solveLinearSystem_(A, b, x, s, t)
            M = A.conj().T if t else A
            res = np.linalg.norm(M @ x - b) / np.linalg.norm(b)
            print(f"  doTranspose = {t}: {s.nIter} iterations in all, flag {p.flag}, true residual {res:.2e}")
            assert p.doTranspose == t and p.flag in (0, -3) and res < s.tol      # (the assertion of tests/test_complex_krylov_gpu.py)
            if dev is None:
                dev = p.device
            assert dev is not None and p.device is dev
    finally:
        mg.clear_(p)
