"""-m gpu: replaceMatrixInHierarchy of ComplexF32 hierarchies on the MI355X (a param with ``singleDeviceSetup=True``: mg_rap_CF32,
mg_get_values_CF32, mg_get_relax_CF32, mg_replace_values_CF32, mg_rap_level_ms_CF32).

Bounds.  Products and relaxPrecs: the yardsticks of tests/complex_single_rap_cases.py (one rounding to single of the ComplexF64 sum
of the read-back operators: 2^-24 |ref| + 1e-13 max|ref| per part; relaxPrecs 2^-23 |ref|).  Cycles: the bound of the header of
tests/test_complex_single_gpu.py - the device's distance from its comparand is at most 4 e_ref, e_ref the single numpy restatement's
distance from the complex128 oracle cycle on the same hierarchy widened, computed in the test.  Stream kernel: the row bound of that
file, (m_i + 8) 2^-24 sum_k |a_ik||x_k|.  Shapes: those tests/test_complex_rap_gpu.py established for the ComplexF64 twin."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import complex_oracle as corc
import complex_single_oracle as cs
import complex_single_rap_cases as SR
import complex_vanka_cases as CV
from complex_cases import complex_rhs, helmholtz

pytestmark = pytest.mark.gpu

MG_ERR_INVALID, MG_ERR_STATE, MG_ERR_UNSUPPORTED = 1, 3, 4
C64, U32 = SR.C64, SR.U32
FP, DP = C.POINTER(C.c_float), C.POINTER(C.c_double)


def _rhs32(n, seed):
    return complex_rhs(n, seed).astype(C64)


def _e_ref(p, b):
    """The single restatement's distance from the complex128 oracle cycle on the widened hierarchy, one cycle from zero."""
    xs = cs.recursiveCycle(p, b, np.zeros_like(b), 1)
    xo = corc.recursiveCycle(cs.rounded(p), b.astype(np.complex128), np.zeros(b.shape[0], dtype=np.complex128), 1)
    return cs.rel2(xs, xo), xs, xo


# ---- 1. the device path against the yardstick ------------------------------------------------------------------------------------
@pytest.mark.parametrize("relaxType,omega,cells,chunk,groups", [("Jac", 0.8, [16, 16, 16], 0, 0), ("SPAI", 1.0, [24, 20], 0, 0),
                                                                ("Jac", 0.8, [12, 12, 12], 10, 0), ("SPAI", 1.0, [12, 12, 12], 10, 1),
                                                                ("Jac", 0.8, [24, 20], 0, 16)])
def test_replace_matrix_on_device_against_the_yardstick(mg, built, monkeypatch, relaxType, omega, cells, chunk, groups):
    if chunk:
        monkeypatch.setenv("MG_RAP_CHUNK", str(chunk))
    if groups:
        monkeypatch.setenv("MG_RAP_GROUPS", str(groups))
    A, mesh = helmholtz(mg, cells, 0.5, 0.5)
    p = SR.single_param(mg, 3, relaxType, omega)
    mg.MGsetup(A, mesh, p)
    b = _rhs32(A.shape[0], 9)
    mg.solveMG(p, b, np.zeros_like(b))                    # uploads the hierarchy
    dev_before = p.device
    assert isinstance(dev_before, mg.device.ComplexSingleDeviceHierarchy)
    patterns = [(M.indptr.copy(), M.indices.copy()) for M in p.As]
    A2 = SR.new_matrix(A, 8)
    mg.replaceMatrixInHierarchy(p, A2)
    assert p.device is dev_before                         # stayed resident: the device path was taken
    for (ip, ix), M in zip(patterns, p.As):
        assert np.array_equal(ip, M.indptr) and np.array_equal(ix, M.indices) and M.dtype == C64
    assert p.As[0].data.tobytes() == A2.data.tobytes()
    if chunk:
        assert max(np.diff(M.indptr).max() for M in p.As[1:]) > chunk
    SR.assert_refreshed(mg, p, relaxType, omega)
    x = np.zeros_like(b)
    _, _, it = mg.solveMG(p, b, x)
    hist = {}
    _, ito = cs.solveMG(p, b, np.zeros_like(b), hist)
    rvo = hist["resvec"]
    e_ref, _, _ = _e_ref(p, b)
    k = min(len(rvo), len(p.resvec))
    d = np.abs(p.resvec[:k] - rvo[:k]).max() / rvo[0]
    print(f"  solveMG after the replacement: {it} cycles ({ito}), resvec diff {d:.3e} of resvec[0] (allowed {4 * e_ref:.3e}), "
          f"reduction {p.resvec[-1] / p.resvec[0]:.2e}")
    assert d <= 4 * e_ref and abs(it - ito) <= 1
    assert p.resvec[-1] < p.resvec[0]
    # deterministic (no atomics, ordered column sums): a second pass over the same values gives the same bits
    first = [M.data.copy() for M in p.As[1:]]
    first_d = [np.array(d, copy=True) for d in p.relaxPrecs[:len(p.As) - 1]]
    mg.replaceMatrixInHierarchy(p, A2)
    assert p.device is dev_before
    for v0, M in zip(first, p.As[1:]):
        assert v0.tobytes() == M.data.tobytes()
    for d0, d in zip(first_d, p.relaxPrecs):
        assert d0.tobytes() == d.tobytes()
    mg.clear_(p)


# ---- 2. the C ABI on the awkward operator ----------------------------------------------------------------------------------------
def _row_bound(M, x):
    """(m_i + 8) 2^-24 sum_k |a_ik||x_k| (alpha = 1, beta = 0), in double"""
    absM = sp.csr_matrix((np.abs(M.data.astype(np.complex128)), M.indices, M.indptr), shape=M.shape)
    return (np.diff(M.indptr) + 8) * U32 * (absM @ np.abs(x.astype(np.complex128)))


def test_c_abi_on_an_awkward_operator(mg, built):
    n, nc = 5000, 700
    D = mg.device
    pat = SR.awkward_pattern(n, 3)
    P0 = sp.random(n, nc, density=4.0 / nc, random_state=7, format="csr").astype(np.float32)
    R0 = sp.random(nc, n, density=6.0 / n, random_state=8, format="csr").astype(np.float32)
    P0.sort_indices()
    R0.sort_indices()
    assert (np.diff(P0.indptr) == 0).any() and (np.diff(R0.indptr) == 0).any()       # empty rows in P and R too
    A0 = SR.values(pat, 1, True)
    Cpat = (abs(R0) @ (abs(pat) @ abs(P0))).tocsr()                                # the structural product
    Cpat.sort_indices()
    assert (np.diff(Cpat.indptr) == 0).any() and np.diff(Cpat.indptr).max() > 5 * 64   # empty rows; rows of many passes of 64
    rng = np.random.default_rng(2)
    d0 = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(C64)
    Ac0 = SR.values(Cpat, 4, True)
    p = SR.manual_param(mg, A0, P0, R0, Ac0, d0)
    lib = D.load_library()
    dev = D.DeviceHierarchy(p, options={"rap_chunk": 64})
    assert isinstance(dev, D.ComplexSingleDeviceHierarchy)
    wide = None
    Ah, meshh = helmholtz(mg, [8, 8, 8], 0.5, 0.5)
    pd = mg.getMGparam(np.complex128, np.int64, 2, 8, 4, 1e-10, "Jac", 0.8, 1, 1, "V")
    mg.MGsetup(Ah, meshh, pd)
    ddev = D.DeviceHierarchy(pd)                                                  # a CF64 handle
    A8, mesh8 = mg.poisson_shifted([8, 8, 8])
    pr = mg.getMGparam(np.float64, np.int64, 2, 8, 4, 1e-10, "Jac", 0.8, 1, 1, "V")
    mg.MGsetup(A8, mesh8, pr)
    rdev = D.DeviceHierarchy(pr)                                                  # an FP64 handle
    try:
        h = dev.handle
        done = C.c_longlong(0)
        fp = lambda a: a.ctypes.data_as(FP)
        dp = lambda a: a.ctypes.data_as(DP)
        at = lambda M: np.ascontiguousarray(np.conj(M.data), dtype=C64)              # the reference's AT values
        A1 = SR.values(pat, 11, True)
        om = np.array([0.8, 0.0])
        ms = np.zeros(1)
        assert lib.mg_rap_level_ms_CF32(h, dp(ms), 1) == MG_ERR_STATE and lib.mg_last_error()      # no re-setup yet

        def got_coarse(d):
            return sp.csr_matrix((d.get_values(2, D.MG_OP_A), Cpat.indices, Cpat.indptr), shape=Cpat.shape)

        # -- mg_rap_CF32 + mg_get_values_CF32 + mg_get_relax_CF32, both kinds
        for kind, name in ((0, "Jac"), (1, "SPAI")):
            nz = at(A1)
            assert lib.mg_rap_CF32(h, fp(nz), A1.nnz, kind, dp(om), C.byref(done)) == 0, lib.mg_last_error()
            assert done.value == 1
            fine = dev.get_values(1, D.MG_OP_A)
            assert fine.dtype == C64 and fine.tobytes() == A1.data.tobytes()         # the fine values: conjugated in, conjugated out
            ep = SR.product_excess(got_coarse(dev), R0, A1, P0)
            dgot = np.zeros(n, dtype=C64)
            assert lib.mg_get_relax_CF32(h, 1, fp(dgot), n) == 0, lib.mg_last_error()
            er, finite = SR.relax_excess(mg, dgot, A1, name, 0.8)
            print(f"  {name}: As[2] {ep:.3f} of its bound, relaxPrec {er:.3f} of its bound ({finite} finite)")
            assert finite >= n - 40 and (kind == 1 or finite == n - 40)
            assert ep <= 1.0 and er <= 1.0
        # -- the device time of the last re-setup
        assert lib.mg_rap_level_ms_CF32(h, dp(ms), 1) == 0, lib.mg_last_error()
        assert 0.0 < ms[0] < 1e4 and np.array_equal(dev.rap_level_ms(), ms)
        assert lib.mg_rap_level_ms_CF32(h, dp(ms), 2) == MG_ERR_INVALID and lib.mg_last_error()
        assert lib.mg_rap_level_ms_CF32(h, None, 1) == MG_ERR_INVALID
        # -- the default options: rows of 700 target columns in one pass, the lane groups cut down to what fits the LDS
        dflt = D.DeviceHierarchy(p)
        try:
            nz = at(A1)
            assert lib.mg_rap_CF32(dflt.handle, fp(nz), A1.nnz, 0, dp(om), None) == 0, lib.mg_last_error()
            ep = SR.product_excess(got_coarse(dflt), R0, A1, P0)
            print(f"  default options: As[2] {ep:.3f} of its bound")
            assert ep <= 1.0
        finally:
            dflt.close()
        # -- mg_replace_values_CF32 + mg_spmv_CF32 for A, P and R
        A2, P2, R2 = SR.values(pat, 12, True), SR.values(P0, 13, False), SR.values(R0, 14, False)
        dev.replace_values(1, D.MG_OP_A, A2)
        dev.replace_values(1, D.MG_OP_P, P2)
        dev.replace_values(1, D.MG_OP_R, R2)
        gp, gr = dev.get_values(1, D.MG_OP_P), dev.get_values(1, D.MG_OP_R)
        assert gp.dtype == np.float32 and gp.tobytes() == P2.data.tobytes() and gr.tobytes() == R2.data.tobytes()
        for which, M in ((D.MG_OP_A, A2), (D.MG_OP_P, P2), (D.MG_OP_R, R2)):
            x = _rhs32(M.shape[1], 20 + which)
            y = np.zeros(M.shape[0], dtype=C64)
            dev.spmv(1, which, 1.0, x, 0.0, y)
            want = M.astype(np.complex128) @ x.astype(np.complex128)
            bound = _row_bound(M, x)
            err = np.abs(y.astype(np.complex128) - want)
            nzr = bound > 0
            print(f"  spmv after replace_values({which}): worst row {float((err[nzr] / bound[nzr]).max()):.3f} of its bound")
            assert np.all(err[~nzr] == 0.0) and np.all(err[nzr] <= bound[nzr])

        # -- refusals: the code and a message, nothing written
        def refused(rc, code):
            assert rc == code, (rc, lib.mg_last_error())
            assert lib.mg_last_error()

        keep = [dev.get_values(1, w).copy() for w in (D.MG_OP_A, D.MG_OP_P, D.MG_OP_R)] + [dev.get_values(2, D.MG_OP_A).copy()]
        dkeep = np.zeros(n, dtype=C64)
        assert lib.mg_get_relax_CF32(h, 1, fp(dkeep), n) == 0
        nz = at(A1)
        refused(lib.mg_rap_CF32(None, fp(nz), A1.nnz, 0, dp(om), None), MG_ERR_INVALID)
        refused(lib.mg_rap_CF32(h, None, A1.nnz, 0, dp(om), None), MG_ERR_INVALID)
        refused(lib.mg_rap_CF32(h, fp(nz), A1.nnz, 0, None, None), MG_ERR_INVALID)
        refused(lib.mg_rap_CF32(h, fp(nz), A1.nnz - 1, 0, dp(om), None), MG_ERR_INVALID)            # wrong nnz
        refused(lib.mg_rap_CF32(h, fp(nz), A1.nnz, 2, dp(om), None), MG_ERR_INVALID)                # a bad relaxKind
        fz = np.zeros(2 * max(Ah.nnz, A8.nnz) + 2, dtype=np.float32)
        for hh, M in ((ddev.handle, Ah), (rdev.handle, A8)):                                        # a CF64 and an FP64 handle
            refused(lib.mg_rap_CF32(hh, fp(fz), M.nnz, 0, dp(om), None), MG_ERR_STATE)
            refused(lib.mg_rap_level_ms_CF32(hh, dp(ms), 1), MG_ERR_STATE)
            refused(lib.mg_get_values_CF32(hh, 1, 0, fp(fz), M.nnz), MG_ERR_STATE)
            refused(lib.mg_get_relax_CF32(hh, 1, fp(fz), M.shape[0]), MG_ERR_STATE)
            refused(lib.mg_replace_values_CF32(hh, 1, 0, fp(fz), M.nnz), MG_ERR_STATE)
        dz = np.zeros(2 * A1.nnz)
        refused(lib.mg_rap_CF64(h, dp(dz), A1.nnz, 0, dp(om), None), MG_ERR_UNSUPPORTED)             # the _CF64 forms keep refusing it
        refused(lib.mg_rap_level_ms_CF64(h, dp(ms), 1), MG_ERR_UNSUPPORTED)
        refused(lib.mg_get_values_CF64(h, 1, 0, dp(dz), A1.nnz), MG_ERR_UNSUPPORTED)
        refused(lib.mg_get_relax_CF64(h, 1, dp(dz), n), MG_ERR_UNSUPPORTED)
        refused(lib.mg_replace_values_CF64(h, 1, 0, dp(dz), A1.nnz), MG_ERR_UNSUPPORTED)
        refused(lib.mg_get_values_CF32(h, 1, 0, fp(nz), A1.nnz + 1), MG_ERR_INVALID)
        refused(lib.mg_get_values_CF32(h, 1, 0, None, A1.nnz), MG_ERR_INVALID)
        refused(lib.mg_get_values_CF32(h, 2, D.MG_OP_P, fp(nz), 1), MG_ERR_INVALID)     # the coarsest level has no transfer operators
        refused(lib.mg_get_relax_CF32(h, 1, fp(nz), n + 1), MG_ERR_INVALID)
        refused(lib.mg_replace_values_CF32(h, 1, D.MG_OP_P, fp(nz), P0.nnz + 1), MG_ERR_INVALID)
        refused(lib.mg_replace_values_CF32(h, 1, 7, fp(nz), A1.nnz), MG_ERR_INVALID)
        wide = D.DeviceHierarchy(p, options={"force_rowptr64": 1})
        refused(lib.mg_rap_CF32(wide.handle, fp(nz), A1.nnz, 0, dp(om), None), MG_ERR_UNSUPPORTED)   # 64-bit row pointers
        # a handle that is not finalized (a relaxPrec was set since): refused, then finalized again with finite relaxPrecs
        dev._set_relax(1, dkeep, 1, 1)
        refused(lib.mg_rap_CF32(h, fp(nz), A1.nnz, 0, dp(om), None), MG_ERR_STATE)
        for w, v0 in zip((D.MG_OP_A, D.MG_OP_P, D.MG_OP_R), keep):                                    # nothing was written
            assert dev.get_values(1, w).tobytes() == v0.tobytes()
        assert dev.get_values(2, D.MG_OP_A).tobytes() == keep[3].tobytes()
        dnow = np.zeros(n, dtype=C64)
        assert lib.mg_get_relax_CF32(h, 1, fp(dnow), n) == 0 and dnow.tobytes() == dkeep.tobytes()
        dev._set_relax(1, d0, 1, 1)
        assert lib.mg_finalize(h) == 0
        # -- the handle still cycles, with the values written last
        p.As[0], p.Ps[0], p.Rs[0] = A2, P2, R2
        b = _rhs32(n, 15)
        x = np.zeros_like(b)
        dev.cycle(b, x, 1)
        e_ref, _, xo = _e_ref(p, b)
        e_dev = cs.rel2(x, xo)
        print(f"  one cycle afterwards: restatement {e_ref:.3e}, device {e_dev:.3e} from the double cycle")
        assert e_dev <= 4 * e_ref
    finally:
        dev.close()
        ddev.close()
        rdev.close()
        if wide is not None:
            wide.close()


# ---- 3. the forms of the coarsest solve ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["inverse", "device_inverse", "gmres"])
def test_replace_matrix_refreshes_the_coarsest_solve(mg, built, form):
    """The resident handle after the replacement against a fresh param set up on the new matrix and uploaded whole, one cycle from zero:
    a stale widened coarsest operator, inverse or Jacobi vector is off by O(1) (the new diagonal differs by 50-150 %)."""
    kw = {"inverse": {}, "device_inverse": {"coarseDeviceInverse": True}, "gmres": {"coarse": "GMRES"}}[form]
    A, mesh = helmholtz(mg, [16, 16, 16], 0.5, 0.5)
    p = SR.single_param(mg, 3, "Jac", 0.8, **kw)
    mg.MGsetup(A, mesh, p)
    b = _rhs32(A.shape[0], 9)
    x_old = np.zeros_like(b)
    mg.recursiveCycle(p, b, x_old)
    dev = p.device
    assert dev is not None and dev._coarse_device_inverse == (form == "device_inverse")
    assert bool(getattr(dev, "_coarse_gmres", False)) == (form == "gmres")
    A2 = SR.new_matrix(A, 11)
    t = {}
    mg.replaceMatrixInHierarchy(p, A2)
    assert p.device is dev
    dev.replace_matrix(p, A2, timings=t)
    assert set(t) >= {"rap", "readback", "coarsest"} and p.device is dev
    SR.assert_refreshed(mg, p, "Jac", 0.8, tag=f"{form} ")
    x = np.zeros_like(b)
    mg.recursiveCycle(p, b, x)
    fresh = SR.single_param(mg, 3, "Jac", 0.8, flag=False, **kw)
    mg.MGsetup(A2, mesh, fresh)
    xf = np.zeros_like(b)
    mg.recursiveCycle(fresh, b, xf)
    assert fresh.device is not dev
    yard = SR.single_param(mg, 3, "Jac", 0.8, flag=False)             # (the restatement solves the coarsest level with a factorisation)
    mg.MGsetup(A2, mesh, yard)
    e_ref, _, _ = _e_ref(yard, b)
    e = cs.rel2(x, xf)
    print(f"  {form}: resident against fresh {e:.3e} (allowed {4 * e_ref:.3e}); against the cycle before the replacement {cs.rel2(x, x_old):.2e}")
    assert e <= 4 * e_ref
    assert cs.rel2(x, x_old) > 0.05                                   # (the matrix did change)
    mg.clear_(p)
    mg.clear_(fresh)


# ---- 4. Vanka in single ----------------------------------------------------------------------------------------------------------
def _vanka_param(mg, n, omega, **kw):
    p = mg.getMGparam(np.complex128, np.int64, 3, 1, 3, 1e-30, "VankaFaces", CV.W, 1, 1, "V", "NoMUMPS", 0.4, 0.0,
                      "SystemsFacesMixedLinear", singlePrecision=True, complexVanka=True, singleDeviceSetup=True, **kw)
    mg.MGsetup(CV.operator(n, omega), CV.mesh(mg, n), p)
    assert p.levels == 3
    return p


def test_vanka_single_stays_on_the_device(mg, built):
    n, _, omega, _ = CV.CASES["24v"]                                   # the smallest three-level case
    q = _vanka_param(mg, n, omega, vankaDeviceSetup=True)
    A = q.As[0]
    b = CV.rhs(A.shape[0], True)
    mg.recursiveCycle(q, b, np.zeros_like(b))
    dev = q.device
    assert isinstance(dev, mg.device.ComplexSingleDeviceHierarchy) and dev._vanka_device_setup
    A2 = sp.csr_matrix(A.astype(np.complex128) * (2 - 0.5j)).astype(C64)
    t = {}
    mg.replaceMatrixInHierarchy(q, A2)
    assert q.device is dev                                             # the handle stays resident
    dev.replace_matrix(q, A2, timings=t)
    assert set(t) >= {"rap", "readback", "coarsest", "blocks_readback"}
    vtype = CV.VTYPES["VankaFaces"]
    for l in range(q.levels - 1):
        again = mg.setupVankaFacesPreconditioner(q.As[l], q.Meshes[l], CV.W, True, vtype, device=True)
        assert q.relaxPrecs[l].dtype == C64 and q.relaxPrecs[l].shape == again.shape
        assert q.relaxPrecs[l].tobytes(order="F") == again.tobytes(order="F")       # the same kernel on the same values
        ep = SR.product_excess(q.As[l + 1], q.Rs[l], q.As[l], q.Ps[l])
        print(f"  level {l + 1}: blocks identical, As[{l + 2}] {ep:.3f} of its bound")
        assert ep <= 1.0
    x = np.zeros_like(b)
    mg.recursiveCycle(q, b, x)
    Hs, Ho = CV.Hier(q), CV.Hier(q, widen=True)
    xs = CV.restate_cycle(Hs, b, None, True, "V")
    xo = CV.restate_cycle(Ho, b.astype(np.complex128), None, True, "V")
    e_ref, e_dev = CV.rel2(xs, xo), CV.rel2(x, xo)
    print(f"  one cycle on the refreshed param: restatement {e_ref:.3e}, device {e_dev:.3e} from the complex128 cycle")
    assert q.device is dev and e_dev <= 4 * e_ref
    # -- the refusals of mg_rap_CF32 on a Vanka handle, before the first write
    lib = mg.device.load_library()
    nz = np.ascontiguousarray(np.conj(A2.data), dtype=C64)
    om = np.full(q.levels, 0.6)
    rap = lambda hd: lib.mg_rap_CF32(hd, nz.ctypes.data_as(FP), A2.nnz, 0, om.ctypes.data_as(DP), None)
    before = dev.get_values(2, mg.device.MG_OP_A).copy()
    assert lib.mg_set_option(dev.handle, b"vanka_device_setup", 0.0) == 0
    assert rap(dev.handle) == MG_ERR_UNSUPPORTED and b"set up on the host" in lib.mg_last_error()
    assert lib.mg_set_option(dev.handle, b"vanka_device_setup", 1.0) == 0
    assert rap(dev.handle) == 0, lib.mg_last_error()
    assert dev.get_values(2, mg.device.MG_OP_A).tobytes() == before.tobytes()
    host = _vanka_param(mg, n, omega)                                  # blocks bound by mg_set_vanka_CF32: nothing remembered
    mg.recursiveCycle(host, b, np.zeros_like(b))
    hdev = host.device
    keep = hdev.get_values(1, mg.device.MG_OP_A).copy()
    assert lib.mg_set_option(hdev.handle, b"vanka_device_setup", 1.0) == 0
    assert rap(hdev.handle) == MG_ERR_STATE and lib.mg_last_error()
    assert hdev.get_values(1, mg.device.MG_OP_A).tobytes() == keep.tobytes()
    assert lib.mg_set_option(hdev.handle, b"vanka_device_setup", 0.0) == 0
    # -- without vankaDeviceSetup the call falls back to the host path
    mg.replaceMatrixInHierarchy(host, A2)
    assert host.device is None
    mg.clear_(q)
    mg.clear_(host)


# ---- 5. the loop a user writes ---------------------------------------------------------------------------------------------------
def test_inversion_loop_keeps_the_single_hierarchy_resident(mg, built):
    """Two successive media on one grid: the ComplexF32 hierarchy on the damped operator is refreshed in HBM, the undamped ComplexF64
    Krylov operator gets new values on the pattern uploaded last, BiCGSTAB solves each system."""
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
    p = SR.single_param(mg, 3, "SPAI", 1.0, 2, 1, "V", 60, 1e-8)
    mg.MGsetup(operator(media[0], 0.5), mesh, p)
    b = complex_rhs(n, 21)
    mg.solveBiCGSTAB_MG_CFP64(operator(media[0], 0.05), p, b, np.zeros_like(b))       # uploads the hierarchy and the operator
    dev = p.device
    pat = dev._krylov_pattern
    assert isinstance(dev, mg.device.ComplexSingleDeviceHierarchy) and pat is not None
    for m in media[1:]:
        mg.replaceMatrixInHierarchy(p, operator(m, 0.5))
        assert p.device is dev and p.As[0].dtype == C64
        A_sys = operator(m, 0.05)
        x = np.zeros_like(b)
        _, _, it, _ = mg.solveBiCGSTAB_MG_CFP64(A_sys, p, b, x)
        res = np.linalg.norm(b - A_sys @ x) / np.linalg.norm(b)
        print(f"  medium: {it} iterations, flag {p.flag}, ||b - A x|| / ||b|| = {res:.2e}")
        assert p.device is dev and dev.krylov_operator is A_sys and dev._krylov_pattern is pat
        assert res < 1e-6
    # the auto-widened fine level follows a re-setup too: no Krylov operator set, the drivers apply the NEW As[1]
    dev.set_krylov_operator(None)
    A_last = SR.new_matrix(p.As[0], 5)
    x0 = np.zeros_like(b)
    dev.bicgstab(b, x0, 1e-8, 60)                                                    # widens the present As[1]
    mg.replaceMatrixInHierarchy(p, A_last)
    assert p.device is dev
    x1 = np.zeros_like(b)
    _, flag, it, _ = dev.bicgstab(b, x1, 1e-8, 60)
    res = np.linalg.norm(b - A_last.astype(np.complex128) @ x1) / np.linalg.norm(b)
    print(f"  no Krylov operator: {it} iterations, flag {flag}, ||b - As[1] x|| / ||b|| = {res:.2e}")
    assert res < 1e-6
    mg.clear_(p)
