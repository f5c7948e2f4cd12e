"""-m gpu: the Vanka cell blocks built and refreshed on the device (vanka_build_blocks, csrc/mg_vanka.hpp) - the stand-alone handle,
``setupVankaFacesPreconditioner(..., device=True)``, complex Vanka hierarchies with ``vankaDeviceSetup=True`` and their re-setup in
HBM (mg_rap_CF64 with the option vanka_device_setup).

Bounds.  Blocks against the host function: ``vanka_device_setup_cases.block_excess`` <= 1, i.e. per real or imaginary component
|dev - host| <= spacing32(|host|) + 2^-40 max|host block| (derivation there).  Cycles and solves of a param with the flag against
the same param without it: 1e-11 of max|x| for ComplexF64 (the TOL of tests/test_complex_vanka_gpu.py for complex Vanka cycles)
and 64 * 2^-24 for ``singlePrecision`` (the bound those tests put on a single-precision cycle's distance from its double
comparand); the kernels and operators are the same, only the blocks' origin differs.  As[l] after a re-setup against the host's
Galerkin products: 1e-13 of max|entry|, the bound of tests/test_complex_rap_gpu.py::_assert_refreshed."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import complex_vanka_cases as CV
import vanka_cases as V
import vanka_device_setup_cases as S

pytestmark = pytest.mark.gpu

TOL = {False: 1e-11, True: 64 * 2.0 ** -24}
MG_ERR_INVALID, MG_ERR_STATE, MG_ERR_UNSUPPORTED = 1, 3, 4
_dp = C.POINTER(C.c_double)


def _compare(mg, A, n, ip, label):
    """Every variant of one operator through one handle: upload once, build, read back, compare with the host function."""
    with mg.vanka.vanka_handle(A, None, n, ip, w=S.VARIANTS[0][1], VankaType=S.VARIANTS[0][0]) as H:
        for vtype, w in S.VARIANTS:
            H.build_blocks(w, vtype)
            dev = H.blocks()
            host = mg.setupVankaFacesPreconditioner(A, np.asarray(n), w, ip, vtype)
            assert dev.shape == host.shape and dev.dtype == host.dtype and dev.flags.f_contiguous
            worst, share = S.block_excess(dev, host)
            print(f"{label} type {vtype} w={w}: worst error / bound {worst:.3f}, bits differ in {share:.2e} of the components")
            assert worst <= 1.0


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("n,ip", S.MESHES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else ("p" if v else "f"))
def test_blocks_against_host(mg, built, n, ip, cx):
    _compare(mg, S.operator(n, ip, cx), n, ip, f"{n} ip={ip} cx={cx}")


def test_blocks_absent_couplings(mg, built):
    n, ip = [5, 3, 2], True
    _compare(mg, S.thinned(S.operator(n, ip, True)), n, ip, "thinned [5,3,2]")
    _compare(mg, S.thinned(S.operator(n, ip, False)), n, ip, "thinned real [5,3,2]")


def test_device_argument_of_the_host_function(mg, built):
    """setupVankaFacesPreconditioner(..., device=True): shape, dtype and memory order of the host path; values to the tolerance."""
    n, ip = [5, 3, 2], True
    for cx in (False, True):
        A = S.operator(n, ip, cx)
        host = mg.setupVankaFacesPreconditioner(A, np.asarray(n), (0.6, 0.4), ip, V.FULL_VANKA_ADD)
        dev = mg.setupVankaFacesPreconditioner(A, np.asarray(n), (0.6, 0.4), ip, V.FULL_VANKA_ADD, device=True)
        assert type(dev) is np.ndarray and dev.shape == host.shape and dev.dtype == host.dtype and dev.flags.f_contiguous
        assert S.block_excess(dev, host)[0] <= 1.0
    A32 = S.operator(n, ip, True).astype(np.complex64)       # (a ComplexF32 level's operator: widened, as the host path reads it)
    host = mg.setupVankaFacesPreconditioner(A32, np.asarray(n), 0.6, ip, V.FULL_VANKA_RB)
    dev = mg.setupVankaFacesPreconditioner(A32, np.asarray(n), 0.6, ip, V.FULL_VANKA_RB, device=True)
    assert dev.dtype == np.complex64 and S.block_excess(dev, host)[0] <= 1.0
    with pytest.raises(TypeError):
        mg.setupVankaFacesPreconditioner(A32, np.asarray(n), (0.6, 0.4), ip, V.ECON_VANKA_RB, device=True)
    with pytest.raises(NotImplementedError):
        mg.setupVankaFacesPreconditioner(A32, np.asarray(n), 0.6, ip, V.FULL_VANKA_LEX, device=True)


def test_two_builds_give_the_same_bits(mg, built):
    n, ip = [9, 8, 5], True
    A = S.operator(n, ip, True)
    with mg.vanka.vanka_handle(A, None, n, ip, w=(0.6, 0.4), VankaType=V.FULL_VANKA_ADD) as H:
        first = H.blocks()
        H.build_blocks((0.6, 0.4), V.FULL_VANKA_ADD)
        second = H.blocks()
    with mg.vanka.vanka_handle(A, None, n, ip, w=(0.6, 0.4), VankaType=V.FULL_VANKA_ADD) as H2:
        third = H2.blocks()
    assert first.tobytes(order="F") == second.tobytes(order="F") == third.tobytes(order="F")


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_replace_values_round_trip(mg, built, cx):
    """replace_values(2A) then build_blocks: half the blocks (the scaling by two is exact, so the tolerance is the build's own)."""
    n, ip = [5, 3, 2], True
    A = S.operator(n, ip, cx)
    with mg.vanka.vanka_handle(A, None, n, ip, w=0.6, VankaType=V.FULL_VANKA_ADD) as H:
        before = H.blocks()
        H.replace_values(2.0 * A)
        assert H.blocks().tobytes(order="F") == before.tobytes(order="F")        # (the blocks stay until they are built again)
        H.build_blocks(0.6, V.FULL_VANKA_ADD)
        after = H.blocks()
    host_half = (0.5 * mg.setupVankaFacesPreconditioner(A, np.asarray(n), 0.6, ip, V.FULL_VANKA_ADD)).astype(before.dtype)
    assert S.block_excess(after, np.asfortranarray(host_half))[0] <= 1.0
    assert S.block_excess(after, np.asfortranarray((0.5 * before).astype(before.dtype)))[0] <= 1.0


def test_singular_cell_is_an_error_return(mg, built):
    n, ip = [3, 2, 2], True
    A = S.operator(n, ip, True)
    bad = S.zero_row_of_cell(A, n, ip, cell=5, slot=6)       # (the pressure row: it belongs to this cell alone)
    lib = mg.device.load_library()
    N = A.shape[0]
    x0, b = V.seeded(N, 3, True), V.seeded(N, 4, True)
    w = np.array([0.6, 0.4])
    with mg.vanka.vanka_handle(A, None, n, ip, w=(0.6, 0.4), VankaType=V.FULL_VANKA_RB) as H:
        good = H.blocks()
        H.replace_values(bad)
        assert lib.mg_vanka_build_blocks_CFP64(H.h, V.FULL_VANKA_RB, w.ctypes.data_as(_dp), 2) == MG_ERR_INVALID
        msg = lib.mg_last_error().decode()
        assert "cell 6" in msg and "singular" in msg
        with pytest.raises(np.linalg.LinAlgError):
            H.build_blocks((0.6, 0.4), V.FULL_VANKA_RB)
        assert H.blocks().tobytes(order="F") == good.tobytes(order="F")          # the previous blocks are kept ...
        x = x0.copy()
        mg.RelaxVankaFacesColor(bad, x, b, good, 2, 1, np.asarray(n), ip, V.FULL_VANKA_RB, handle=H)
        ref = x0.copy()
        mg.RelaxVankaFacesColor(bad, ref, b, good, 2, 1, np.asarray(n), ip, V.FULL_VANKA_RB)
        assert np.array_equal(x, ref) and np.all(np.isfinite(x.view(np.float64)))   # ... and relax as a fresh handle with them does
    with pytest.raises(np.linalg.LinAlgError):
        mg.setupVankaFacesPreconditioner(bad, np.asarray(n), (0.6, 0.4), ip, V.FULL_VANKA_RB, device=True)
    with pytest.raises(np.linalg.LinAlgError):
        mg.vanka.vanka_handle(bad, None, n, ip, w=0.6, VankaType=V.FULL_VANKA_ADD)


def test_refusals_of_the_handle(mg, built):
    n, ip = [3, 2], True
    A = S.operator(n, ip, False)
    lib = mg.device.load_library()
    w = np.array([0.6, 0.4])
    with mg.vanka.vanka_handle(A, None, n, ip, w=0.6) as H:
        keep = H.blocks()
        assert lib.mg_vanka_build_blocks_FP64(H.h, V.ECON_VANKA_RB, w.ctypes.data_as(_dp), 2) == MG_ERR_INVALID
        assert lib.mg_vanka_build_blocks_FP64(H.h, 2, w.ctypes.data_as(_dp), 1) == MG_ERR_UNSUPPORTED
        assert lib.mg_vanka_build_blocks_FP64(H.h, V.FULL_VANKA_LEX, w.ctypes.data_as(_dp), 1) == MG_ERR_UNSUPPORTED
        assert lib.mg_vanka_build_blocks_FP64(H.h, 1, w.ctypes.data_as(_dp), 3) == MG_ERR_INVALID
        assert lib.mg_vanka_build_blocks_CFP64(H.h, 1, w.ctypes.data_as(_dp), 1) == MG_ERR_STATE
        assert lib.mg_vanka_replace_values_FP64(H.h, w.ctypes.data_as(_dp), 2) == MG_ERR_INVALID
        assert H.blocks().tobytes(order="F") == keep.tobytes(order="F")


# ---- hierarchies -------------------------------------------------------------------------------------------------------------------
# name -> (cells, levels asked for, omega, levels MGsetup builds).  [8,8,8] asked for three levels stops at two, as in the reference: a
# direction of fewer than 8 cells is not coarsened (Systems.jl:114-164), so 8 -> 4 is its only step; [16,16,16] (16 -> 8 -> 4) is
# the three-level 3-D hierarchy, run once per test where the others run every variant.
HCASES = {"24x16": ([24, 16], 3, 0.15, 3), "8x8x8": ([8, 8, 8], 3, 0.15, 2), "16x16x16": ([16, 16, 16], 3, 0.15, 3)}
SMALL = ["24x16", "8x8x8"]
_params = {}


def _param(mg, name, relaxType="VankaFaces", single=False, flag=False, blocks=False, w=CV.W):
    key = (name, relaxType, single, flag, blocks, w)
    if key not in _params:
        n, levels, omega, built_levels = HCASES[name]
        p = mg.getMGparam(np.complex128, np.int64, levels, 1, 3, 1e-30, relaxType, w, 1, 1, "V", "NoMUMPS", 0.4, 0.0,
                          "SystemsFacesMixedLinear", singlePrecision=single, complexVanka=True, vankaBlocks=blocks,
                          **({"vankaDeviceSetup": True} if flag else {}))
        mg.MGsetup(CV.operator(n, omega), CV.mesh(mg, n), p)
        assert p.levels == built_levels
        _params[key] = p
    return _params[key]


@pytest.mark.parametrize("single", [False, True], ids=["CF64", "CF32"])
@pytest.mark.parametrize("relaxType", ["VankaFaces", "VankaFacesAdd"])
@pytest.mark.parametrize("name", SMALL)
def test_hierarchy_with_the_flag(mg, built, name, relaxType, single):
    p0 = _param(mg, name, relaxType, single)
    p1 = _param(mg, name, relaxType, single, flag=True)
    for l in range(p1.levels - 1):       # relaxPrecs stay ordinary host arrays, built on the device
        assert type(p1.relaxPrecs[l]) is np.ndarray and p1.relaxPrecs[l].dtype == np.complex64
        assert S.block_excess(p1.relaxPrecs[l], p0.relaxPrecs[l])[0] <= 1.0
    b = CV.rhs(p0.As[0].shape[0], single)
    x0, x1 = np.zeros_like(b), np.zeros_like(b)
    mg.recursiveCycle(p0, b, x0)
    mg.recursiveCycle(p1, b, x1)
    e = CV.err_max(x1, x0)
    s0, s1 = np.zeros_like(b), np.zeros_like(b)
    mg.solveMG(p0, b, s0)
    r0 = p0.resvec.copy()
    mg.solveMG(p1, b, s1)
    es = CV.err_max(s1, s0)
    er = np.abs(p1.resvec - r0).max() / r0[0]
    print(f"{name} {relaxType} single={single}: cycle {e:.3e}, solve {es:.3e} of max|x|, residual history {er:.3e}")
    assert p1.device._vanka_device_setup and not p0.device._vanka_device_setup
    assert e <= TOL[single] and es <= TOL[single] and er <= TOL[single]


def test_hierarchy_three_levels_3d(mg, built):
    test_hierarchy_with_the_flag(mg, built, "16x16x16", "VankaFaces", False)


@pytest.mark.parametrize("name", SMALL)
def test_hierarchy_block_of_four(mg, built, name):
    p0 = _param(mg, name, blocks=True)
    p1 = _param(mg, name, blocks=True, flag=True)
    N = p0.As[0].shape[0]
    B = np.asfortranarray(np.stack([V.seeded(N, 20 + j, True) for j in range(4)], axis=1))
    X0, X1 = np.zeros_like(B, order="F"), np.zeros_like(B, order="F")
    mg.recursiveCycle(p0, B, X0)
    mg.recursiveCycle(p1, B, X1)
    e = max(CV.err_max(X1[:, j], X0[:, j]) for j in range(4))
    S0, S1 = np.zeros_like(B, order="F"), np.zeros_like(B, order="F")
    mg.solveMG(p0, B, S0)
    mg.solveMG(p1, B, S1)
    es = max(CV.err_max(S1[:, j], S0[:, j]) for j in range(4))
    print(f"{name} block of 4: cycle {e:.3e}, solve {es:.3e} of max|x| per column")
    assert e <= TOL[False] and es <= TOL[False]


@pytest.mark.parametrize("name,relaxType,w", [("24x16", "VankaFaces", CV.W), ("8x8x8", "VankaFacesAdd", (0.6, 0.4)),
                                              ("16x16x16", "VankaFaces", (0.6, 0.4))])
def test_resetup_stays_on_the_device(mg, built, name, relaxType, w):
    from multigrid_jl_amd.mgsetup import galerkin
    n, asked, omega, levels = HCASES[name]
    A = CV.operator(n, omega)
    q = mg.getMGparam(np.complex128, np.int64, asked, 1, 3, 1e-30, relaxType, w, 1, 1, "V", "NoMUMPS", 0.4, 0.0,
                      "SystemsFacesMixedLinear", complexVanka=True, vankaDeviceSetup=True)
    mg.MGsetup(A, CV.mesh(mg, n), q)
    b = CV.rhs(A.shape[0])
    x = np.zeros_like(b)
    mg.recursiveCycle(q, b, x)
    dev = q.device
    assert dev is not None and q.levels == levels
    A2 = sp.csr_matrix(A * (2 - 0.5j))
    mg.replaceMatrixInHierarchy(q, A2)
    assert q.device is dev                                        # the handle stays resident
    vtype = CV.VTYPES[relaxType]
    Al = sp.csr_matrix(A2)
    for l in range(levels - 1):
        host = mg.setupVankaFacesPreconditioner(q.As[l], q.Meshes[l], w, True, vtype)
        worst, share = S.block_excess(q.relaxPrecs[l], host)
        Al = galerkin(q.Rs[l], Al, q.Ps[l])
        err = np.abs(Al.data - q.As[l + 1].data).max() / np.abs(Al.data).max()
        print(f"{name} level {l + 1}: blocks worst error / bound {worst:.3f} (bits differ in {share:.2e}), As[{l + 2}] {err:.2e} of max|entry|")
        assert np.array_equal(Al.indptr, q.As[l + 1].indptr) and np.array_equal(Al.indices, q.As[l + 1].indices)
        assert err <= 1e-13 and worst <= 1.0
    fresh = mg.getMGparam(np.complex128, np.int64, asked, 1, 3, 1e-30, relaxType, w, 1, 1, "V", "NoMUMPS", 0.4, 0.0,
                          "SystemsFacesMixedLinear", complexVanka=True)
    mg.MGsetup(A2, CV.mesh(mg, n), fresh)
    xf, xq = np.zeros_like(b), np.zeros_like(b)
    mg.recursiveCycle(fresh, b, xf)
    mg.recursiveCycle(q, b, xq)
    e = CV.err_max(xq, xf)
    print(f"{name}: the cycle after the re-setup {e:.3e} of max|x| from a fresh set-up")
    assert q.device is dev and e <= TOL[False]
    t = {}
    dev.replace_matrix(q, A2, timings=t)
    assert set(t) >= {"rap", "readback", "coarsest", "blocks_readback"}
    mg.clear_(q)
    mg.clear_(fresh)


def test_rap_refusals(mg, built):
    """mg_rap_CF64 on a Vanka handle: refused as ever with the option at 0; with it at 1 on levels bound by mg_set_vanka_CF64
    (nothing remembered) MG_ERR_STATE before the first write; a default param still drops its handle on a re-setup."""
    p = _param(mg, "24x16")
    b = CV.rhs(p.As[0].shape[0])
    x = np.zeros_like(b)
    mg.recursiveCycle(p, b, x)
    dev, lib = p.device, mg.device.load_library()
    hd = dev.handle
    nz = np.ascontiguousarray(np.conj((p.As[0] * (2 - 0.5j)).data))
    om = np.full(p.levels, 0.6)
    done = C.c_longlong(0)
    rap = lambda: lib.mg_rap_CF64(hd, nz.ctypes.data_as(_dp), nz.size, 0, om.ctypes.data_as(_dp), C.byref(done))
    assert rap() == MG_ERR_UNSUPPORTED
    assert "set up on the host" in lib.mg_last_error().decode()
    before = dev.get_values(1, mg.device.MG_OP_A)
    assert lib.mg_set_option(hd, b"vanka_device_setup", 1.0) == 0
    assert rap() == MG_ERR_STATE
    assert np.array_equal(dev.get_values(1, mg.device.MG_OP_A), before)
    assert lib.mg_set_option(hd, b"vanka_device_setup", 0.0) == 0
    assert rap() == MG_ERR_UNSUPPORTED
    x2 = np.zeros_like(b)
    mg.recursiveCycle(p, b, x2)
    assert np.array_equal(x, x2)
    # mg_build_vanka_*: the refusals of the stand-alone build, and the other precision's entry
    nn = np.array([24, 16], dtype=np.int64)
    w = np.array([0.6, 0.4])
    lp = C.POINTER(C.c_longlong)
    assert lib.mg_build_vanka_CF64(hd, 1, 2, nn.ctypes.data_as(lp), 1, V.ECON_VANKA_RB, w.ctypes.data_as(_dp), 2) == MG_ERR_INVALID
    assert lib.mg_build_vanka_CF64(hd, 1, 2, nn.ctypes.data_as(lp), 1, 2, w.ctypes.data_as(_dp), 1) == MG_ERR_UNSUPPORTED
    assert lib.mg_build_vanka_CF64(hd, 1, 2, nn.ctypes.data_as(lp), 1, 4, w.ctypes.data_as(_dp), 1) == MG_ERR_UNSUPPORTED
    assert lib.mg_build_vanka_CF32(hd, 1, 2, nn.ctypes.data_as(lp), 1, 1, w.ctypes.data_as(_dp), 1) == MG_ERR_STATE
    x3 = np.zeros_like(b)
    mg.recursiveCycle(p, b, x3)
    assert np.array_equal(x, x3)
    q = mg.getMGparam(np.complex128, np.int64, 3, 1, 3, 1e-30, "VankaFaces", CV.W, 1, 1, "V", "NoMUMPS", 0.4, 0.0,
                      "SystemsFacesMixedLinear", complexVanka=True)
    mg.MGsetup(CV.operator([24, 16], 0.15), CV.mesh(mg, [24, 16]), q)
    mg.recursiveCycle(q, b, np.zeros_like(b))
    assert q.device is not None
    mg.replaceMatrixInHierarchy(q, sp.csr_matrix(q.As[0] * (2 - 0.5j)))
    assert q.device is None
