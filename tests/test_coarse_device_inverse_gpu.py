"""-m gpu: the explicit inverse of the coarsest operator built on the device (csrc/mg_dense_inv.hpp) - the stand-alone inverse
(``device.dense_inverse``), hierarchies with ``coarseDeviceInverse=True``, their re-setup in HBM (mg_rap_* with the option
coarse_device_inverse), the adjoint / transposed hierarchy, and the fall-back to the host route.

Bounds (tests/coarse_inverse_cases.py): an inverse meets res(X) <= 8 * max(res(numpy.linalg.inv(A)), n * eps); cycles and solves
of a param with the flag stay within 1e-11 of max|x| (64 * 2^-24 for ``singlePrecision``) of the same param without it."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import coarse_inverse_cases as K

pytestmark = pytest.mark.gpu

MG_ERR_INVALID, MG_ERR_STATE, MG_ERR_UNSUPPORTED = 1, 3, 4
_dp = C.POINTER(C.c_double)


# ---- the stand-alone inverse ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_standalone_inverse(mg, built, cx):
    worst = 0.0
    for n in K.SIZES:
        A = K.matrix(n, cx)
        X = mg.device.dense_inverse(A)
        assert X.shape == A.shape and X.dtype == A.dtype and X.flags.f_contiguous
        ratio = K.inverse_ratio(A, X)
        worst = max(worst, ratio)
        print(f"n={n} cx={cx}: res {K.res(A, X):.3e}, res / max(res numpy, n eps) = {ratio:.3f}")
        assert ratio <= 8.0
    print(f"cx={cx}: worst ratio {worst:.3f}")


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_exact_case(mg, built, cx):
    """A permutation times a diagonal of signed powers of two: the pivot bookkeeping and the final permutation, nothing rounds."""
    for n in (5, 70, 130):
        A, X = K.exact_case(n, cx)
        got = mg.device.dense_inverse(A)
        assert np.array_equal(got, X), f"n={n}: {np.count_nonzero(got != X)} entries differ"


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_two_runs_give_the_same_bits(mg, built, cx):
    A = K.matrix(200, cx)
    assert mg.device.dense_inverse(A).tobytes(order="F") == mg.device.dense_inverse(A).tobytes(order="F")


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_singular_input_is_an_error_return(mg, built, cx):
    lib = mg.device.load_library()
    Z, N = K.singular_cases(cx)
    fn = lib.mg_dense_inverse_CF64 if cx else lib.mg_dense_inverse_FP64
    out = np.full_like(Z, 7.0, order="F")
    assert fn(0, 70, Z.ctypes.data_as(_dp), out.ctypes.data_as(_dp)) == MG_ERR_INVALID
    assert "column 41" in lib.mg_last_error().decode()          # (1-based)
    assert np.all(out == 7.0)                                   # nothing was returned
    for bad in (Z, N):
        with pytest.raises(np.linalg.LinAlgError):
            mg.device.dense_inverse(bad)
    A = K.matrix(70, cx)                                        # (the library is none the worse for it)
    assert K.inverse_ratio(A, mg.device.dense_inverse(A)) <= 8.0


# ---- hierarchies -----------------------------------------------------------------------------------------------------------------
_params = {}


def _param(mg, name, relaxType="Jac", single=False, flag=False):
    key = (name, relaxType, single, flag)
    if key not in _params:
        A, mesh = K.operator(mg, name)
        p = K.param(mg, name, relaxType, single, flag)
        mg.MGsetup(A, mesh, p)
        _params[key] = p
    return _params[key]


def _is_cx(name):
    return K.HCASES[name][2] == "complex"


def _check_inverse(p, label):
    X = p.device.coarse_dense_inverse()
    Ac = p.As[-1].toarray().astype(np.complex128 if np.iscomplexobj(p.As[-1].data) else np.float64)
    ratio = K.inverse_ratio(Ac, X)
    print(f"{label}: coarsest order {Ac.shape[0]}, res {K.res(Ac, X):.3e}, res / max(res numpy, n eps) = {ratio:.3f}")
    assert ratio <= 8.0
    return X


HIER = [(name, relax, single) for name in K.HCASES for relax in ("Jac", "SPAI") for single in ((False, True) if _is_cx(name) else (False,))]


@pytest.mark.parametrize("name,relaxType,single", HIER, ids=lambda v: str(v))
def test_hierarchy_with_the_flag(mg, built, name, relaxType, single):
    cx = _is_cx(name)
    p0, p1 = _param(mg, name, relaxType, single), _param(mg, name, relaxType, single, flag=True)
    n = p0.As[0].shape[0]
    b = K.rhs(n, cx, single)
    x0, x1 = np.zeros_like(b), np.zeros_like(b)
    mg.recursiveCycle(p0, b, x0)
    mg.recursiveCycle(p1, b, x1)
    assert p1.device._coarse_device_inverse and not p0.device._coarse_device_inverse
    assert p1.device.coarse_form()["kind"] == 0 and p0.device.coarse_form()["kind"] == 0
    _check_inverse(p1, f"{name} {relaxType} single={single}")
    _check_inverse(p0, f"{name} {relaxType} single={single} (host route)")
    e = K.err_max(x1, x0)
    s0, s1 = np.zeros_like(b), np.zeros_like(b)
    mg.solveMG(p0, b, s0)
    r0 = p0.resvec.copy()
    mg.solveMG(p1, b, s1)
    es = K.err_max(s1, s0)
    er = np.abs(p1.resvec - r0).max() / r0[0]
    ek = 0.0
    if cx:
        bk = K.rhs(n, True)
        k0, k1 = np.zeros_like(bk), np.zeros_like(bk)
        mg.solveBiCGSTAB_MG_CFP64(None, p0, bk, k0)
        mg.solveBiCGSTAB_MG_CFP64(None, p1, bk, k1)
        ek = K.err_max(k1, k0)
    print(f"{name} {relaxType} single={single}: cycle {e:.3e}, solveMG {es:.3e}, BiCGSTAB {ek:.3e} of max|x|, residual history {er:.3e}")
    tol = K.TOL[single]
    assert e <= tol and es <= tol and er <= tol and ek <= tol


def test_block_cycle_of_four(mg, built):
    p0, p1 = _param(mg, "8x8x8"), _param(mg, "8x8x8", flag=True)
    n = p0.As[0].shape[0]
    B = np.asfortranarray(np.stack([K.rhs(n, True, seed=20 + j) for j in range(4)], axis=1))
    X0, X1 = np.zeros_like(B, order="F"), np.zeros_like(B, order="F")
    mg.to_device(p0).block_cycle(B, X0, 1)
    mg.to_device(p1).block_cycle(B, X1, 1)
    e = max(K.err_max(X1[:, j], X0[:, j]) for j in range(4))
    print(f"8x8x8 block of 4: cycle {e:.3e} of max|x| per column")
    assert p1.device._coarse_device_inverse and np.abs(X0).max() > 0 and e <= K.TOL[False]


def test_singular_coarsest_operator_keeps_the_inverse(mg, built):
    """The coarsest A zeroed in HBM: the build is refused by its flag (MG_ERR_INVALID) and the next cycle has its old bits."""
    lib = mg.device.load_library()
    for name, fn in (("8x8", lib.mg_build_coarse_dense_inverse_CF64), ("real8x8x8", lib.mg_build_coarse_dense_inverse_FP64)):
        A, mesh = K.operator(mg, name)
        p = K.param(mg, name, flag=True)
        mg.MGsetup(A, mesh, p)
        b = K.rhs(A.shape[0], _is_cx(name))
        x = np.zeros_like(b)
        mg.recursiveCycle(p, b, x)
        dev = p.device
        before = dev.coarse_dense_inverse()
        dev.replace_values(p.levels, mg.device.MG_OP_A, p.As[-1] * 0.0)
        assert fn(dev.handle) == MG_ERR_INVALID
        msg = lib.mg_last_error().decode()
        assert "singular" in msg and "column 1" in msg
        assert dev.coarse_dense_inverse().tobytes(order="F") == before.tobytes(order="F")
        x2 = np.zeros_like(b)
        mg.recursiveCycle(p, b, x2)
        assert p.device is dev and np.array_equal(x, x2)
        mg.clear_(p)


# ---- re-setup ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["8x8x8", "real8x8x8"])
@pytest.mark.parametrize("flag", [True, False], ids=["flag", "default"])
def test_resetup(mg, built, name, flag):
    cx = _is_cx(name)
    A, mesh = K.operator(mg, name)
    q = K.param(mg, name, "SPAI", flag=flag)
    mg.MGsetup(A, mesh, q)
    b = K.rhs(A.shape[0], cx)
    x = np.zeros_like(b)
    mg.recursiveCycle(q, b, x)
    dev = q.device
    assert dev._coarse_device_inverse == flag
    A2, _ = K.operator(mg, name, damping=0.3, shift=2.5)
    mg.replaceMatrixInHierarchy(q, A2)
    assert q.device is dev and dev._coarse_device_inverse == flag      # the handle stays resident, on the same route
    _check_inverse(q, f"{name} flag={flag} after the re-setup")
    assert hasattr(q.LU, "solve")                                      # param.LU stays the host's factorisation
    fresh = K.param(mg, name, "SPAI")
    mg.MGsetup(A2, mesh, fresh)
    xf, xq = np.zeros_like(b), np.zeros_like(b)
    mg.recursiveCycle(fresh, b, xf)
    mg.recursiveCycle(q, b, xq)
    e = K.err_max(xq, xf)
    print(f"{name} flag={flag}: the cycle after the re-setup {e:.3e} of max|x| from a fresh set-up")
    assert q.device is dev and e <= K.TOL[False]
    if cx:
        t = {}
        dev.replace_matrix(q, A2, timings=t)
        assert set(t) >= {"rap", "readback", "coarsest"}
    mg.clear_(q)
    mg.clear_(fresh)


def test_resetup_of_a_vanka_hierarchy(mg, built):
    import complex_vanka_cases as CV
    n, omega = [24, 16], 0.15
    A = CV.operator(n, omega)
    mk = lambda **kw: mg.getMGparam(np.complex128, np.int64, 3, 1, 3, 1e-30, "VankaFaces", CV.W, 1, 1, "V", "NoMUMPS", 0.4, 0.0,
                                    "SystemsFacesMixedLinear", complexVanka=True, **kw)
    q = mk(vankaDeviceSetup=True, coarseDeviceInverse=True)
    mg.MGsetup(A, CV.mesh(mg, n), q)
    b = CV.rhs(A.shape[0])
    x = np.zeros_like(b)
    mg.recursiveCycle(q, b, x)
    dev = q.device
    assert dev._coarse_device_inverse and dev._vanka_device_setup
    A2 = sp.csr_matrix(A * (2 - 0.5j))
    mg.replaceMatrixInHierarchy(q, A2)
    assert q.device is dev and dev._coarse_device_inverse
    _check_inverse(q, "Vanka 24x16 after the re-setup")
    fresh = mk()
    mg.MGsetup(A2, CV.mesh(mg, n), fresh)
    xf, xq = np.zeros_like(b), np.zeros_like(b)
    mg.recursiveCycle(fresh, b, xf)
    mg.recursiveCycle(q, b, xq)
    e = CV.err_max(xq, xf)
    print(f"Vanka 24x16: the cycle after the re-setup {e:.3e} of max|x| from a fresh set-up")
    assert e <= K.TOL[False]
    mg.clear_(q)
    mg.clear_(fresh)


# ---- adjoint and transpose -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["8x8x8", "real8x8x8"])
def test_flipped_hierarchy(mg, built, name):
    cx = _is_cx(name)
    A, mesh = K.operator(mg, name)
    ps = []
    for flag in (False, True):
        p = K.param(mg, name, flag=flag)
        mg.MGsetup(A, mesh, p)
        b = K.rhs(A.shape[0], cx)
        x = np.zeros_like(b)
        mg.recursiveCycle(p, b, x)
        dev = p.device
        (mg.adjointHierarchy if cx else mg.transposeHierarchy)(p)
        assert p.device is dev and dev._coarse_device_inverse == flag     # flipped in HBM, whoever built the inverse
        x = np.zeros_like(b)
        mg.recursiveCycle(p, b, x)
        ps.append((p, x))
    e = K.err_max(ps[1][1], ps[0][1])
    Ac = ps[1][0].As[-1].toarray()
    ratio = K.inverse_ratio(Ac, ps[1][0].device.coarse_dense_inverse())
    print(f"{name}: the cycle of the flipped hierarchy {e:.3e} of max|x| from the flag-off twin; flipped inverse ratio {ratio:.3f}")
    assert e <= K.TOL[False] and ratio <= 8.0
    for p, _ in ps:
        mg.clear_(p)


# ---- fall-back ---------------------------------------------------------------------------------------------------------------------
def test_fall_back_to_the_host_route(mg, built, monkeypatch):
    """coarse_device_inverse_max = 100: the 125-row case takes the host route and has the bits of the flag-off param."""
    monkeypatch.setenv("MG_COARSE_DEVICE_INVERSE_MAX", "100")
    lib = mg.device.load_library()
    A, mesh = K.operator(mg, "8x8x8")
    xs = []
    for flag in (False, True):
        p = K.param(mg, "8x8x8", flag=flag)
        mg.MGsetup(A, mesh, p)
        b = K.rhs(A.shape[0], True)
        x = np.zeros_like(b)
        mg.recursiveCycle(p, b, x)
        assert not p.device._coarse_device_inverse
        if flag:
            before = p.device.coarse_dense_inverse()
            assert lib.mg_build_coarse_dense_inverse_CF64(p.device.handle) == MG_ERR_UNSUPPORTED
            assert "coarse_device_inverse_max" in lib.mg_last_error().decode()
            assert p.device.coarse_dense_inverse().tobytes(order="F") == before.tobytes(order="F")
            x2 = np.zeros_like(b)
            mg.recursiveCycle(p, b, x2)
            assert np.array_equal(x, x2)
        xs.append(x)
        mg.clear_(p)
    assert np.array_equal(xs[0], xs[1])


def test_refusals(mg, built):
    """The value type of the handle, a coarsest solve that is not a dense inverse, the wrong order."""
    lib = mg.device.load_library()
    p = _param(mg, "8x8")
    b = K.rhs(p.As[0].shape[0], True)
    mg.recursiveCycle(p, b, np.zeros_like(b))
    h = p.device.handle
    out = np.zeros((25, 25), dtype=np.complex128, order="F")
    assert lib.mg_build_coarse_dense_inverse_FP64(h) == MG_ERR_STATE
    assert lib.mg_get_coarse_dense_inverse_FP64(h, 25, out.ctypes.data_as(_dp)) == MG_ERR_STATE
    assert lib.mg_get_coarse_dense_inverse_CF64(h, 24, out.ctypes.data_as(_dp)) == MG_ERR_INVALID
    assert lib.mg_get_coarse_dense_inverse_CF64(h, 25, None) == MG_ERR_INVALID
    A, mesh = K.operator(mg, "8x8")
    g = mg.getMGparam(np.complex128, np.int64, 2, 1, 4, 1e-30, "Jac", 0.8, 2, 1, "V", "GMRES")
    mg.MGsetup(A, mesh, g)
    mg.recursiveCycle(g, b, np.zeros_like(b))
    assert lib.mg_get_coarse_dense_inverse_CF64(g.device.handle, 25, out.ctypes.data_as(_dp)) == MG_ERR_STATE
    with pytest.raises(mg.device.MGDeviceError):
        g.device.coarse_dense_inverse()
    mg.clear_(g)
