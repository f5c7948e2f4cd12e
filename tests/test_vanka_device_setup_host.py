"""-m "not gpu": the device set-up of the Vanka blocks, as far as it goes without a device - the numpy restatement of the kernel's
elimination (tests/vanka_device_setup_cases.py) against setupVankaFacesPreconditioner under the tolerance of the GPU comparison,
the new flag of getMGparam, the exported symbols with their ctypes signatures, and the host path's bits."""
import ctypes

import numpy as np
import pytest

import vanka_cases as V
import vanka_device_setup_cases as S

NEW_SYMBOLS = ["mg_vanka_create_built_FP64_INT64", "mg_vanka_create_built_CFP64_INT64", "mg_vanka_build_blocks_FP64",
               "mg_vanka_build_blocks_CFP64", "mg_vanka_replace_values_FP64", "mg_vanka_replace_values_CFP64", "mg_vanka_get_blocks",
               "mg_vanka_time_build", "mg_build_vanka_CF64", "mg_build_vanka_CF32", "mg_get_vanka_blocks_CF64", "mg_get_vanka_blocks_CF32"]


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("n,ip", S.MESHES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else ("p" if v else "f"))
def test_restatement_against_host(mg, n, ip, cx):
    """The kernel's algorithm in numpy gives the host function's blocks within the tolerance of the device comparison."""
    A = S.operator(n, ip, cx)
    for vtype, w in S.VARIANTS:
        host = mg.setupVankaFacesPreconditioner(A, np.asarray(n), w, ip, vtype)
        mine = S.restate_blocks(A, n, w, ip, vtype)
        assert mine.shape == host.shape and mine.dtype == host.dtype and mine.flags.f_contiguous
        worst, share = S.block_excess(mine, host)
        print(f"{n} ip={ip} cx={cx} type {vtype} w={w}: worst error / bound {worst:.3f}, bits differ in {share:.2e} of the components")
        assert worst <= 1.0


def test_restatement_absent_couplings(mg):
    """About a third of the off-diagonal pattern removed: absent in-block couplings are zeros of Acc."""
    n, ip = [5, 3, 2], True
    A = S.thinned(S.operator(n, ip, True))
    full = S.operator(n, ip, True)
    assert 0.55 * full.nnz < A.nnz < 0.85 * full.nnz and np.all(A.diagonal() != 0)
    Acc, AccFull = S.gather(A, n, ip), S.gather(full, n, ip)
    assert np.count_nonzero(Acc) < np.count_nonzero(AccFull)          # couplings inside the blocks are among the removed ones
    for vtype, w in S.VARIANTS:
        host = mg.setupVankaFacesPreconditioner(A, np.asarray(n), w, ip, vtype)
        worst, share = S.block_excess(S.restate_blocks(A, n, w, ip, vtype), host)
        print(f"thinned type {vtype} w={w}: worst error / bound {worst:.3f}, bits differ in {share:.2e}")
        assert worst <= 1.0


def test_restatement_singular_cell(mg):
    n, ip = [3, 2, 2], True
    A = S.zero_row_of_cell(S.operator(n, ip, True), n, ip)
    with pytest.raises(np.linalg.LinAlgError):
        S.restate_blocks(A, n, (0.6, 0.4), ip, V.FULL_VANKA_RB)
    with pytest.raises(np.linalg.LinAlgError):
        mg.setupVankaFacesPreconditioner(A, np.asarray(n), (0.6, 0.4), ip, V.FULL_VANKA_RB)


def _param(mg, **kw):
    return mg.getMGparam(np.complex128, np.int64, 3, 1, 5, 1e-30, "VankaFaces", 0.6, 1, 1, "V", "NoMUMPS", 0.4, 0.0,
                         "SystemsFacesMixedLinear", **kw)


def test_flag_is_accepted(mg):
    """(fails before the flag existed: getMGparam knew no such keyword)"""
    p = _param(mg, complexVanka=True, vankaDeviceSetup=True)
    assert p.vankaDeviceSetup is True and p.complexVanka is True
    ps = _param(mg, complexVanka=True, vankaDeviceSetup=True, singlePrecision=True, vankaBlocks=True)
    assert ps.vankaDeviceSetup and ps.singlePrecision and ps.vankaBlocks
    assert _param(mg, complexVanka=True).vankaDeviceSetup is False
    assert mg.copySolver(p).vankaDeviceSetup is True


def test_flag_needs_complex_vanka(mg):
    with pytest.raises(NotImplementedError):
        _param(mg, vankaDeviceSetup=True)
    with pytest.raises(NotImplementedError):
        mg.getMGparam(np.float64, np.int64, 3, 1, 5, 1e-8, "VankaFaces", 0.6, 1, 1, "V", "NoMUMPS", 0.4, 0.0,
                      "SystemsFacesMixedLinear", vankaDeviceSetup=True)


def test_symbols_and_signatures(mg, built):
    lib = ctypes.CDLL(mg.device.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in mg.device.SIGNATURES
    bound = mg.device.load_library()
    ll, dp, fp, vp = ctypes.c_longlong, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.c_void_p
    assert bound.mg_vanka_build_blocks_CFP64.argtypes == [vp, ll, dp, ll]
    assert bound.mg_vanka_replace_values_FP64.argtypes == [vp, dp, ll]
    assert bound.mg_vanka_get_blocks.argtypes == [vp, fp, ll]
    assert bound.mg_build_vanka_CF32.argtypes == [vp, ll, ll, ctypes.POINTER(ll), ll, ll, dp, ll]
    assert bound.mg_get_vanka_blocks_CF64.argtypes == [vp, ll, fp, ll]
    assert len(bound.mg_vanka_create_built_CFP64_INT64.argtypes) == 12
    for name in NEW_SYMBOLS:
        assert getattr(bound, name).restype == ctypes.c_int
    # a null handle is answered with a status, not a crash, and before any device call
    assert bound.mg_vanka_build_blocks_FP64(None, 1, np.array([0.6]).ctypes.data_as(dp), 1) == 1
    assert bound.mg_vanka_get_blocks(None, None, 0) == 1
    assert bound.mg_get_vanka_blocks_CF64(None, 1, None, 0) != 0


def _host_expected(A, n, w, ip, vtype):
    """The host path written out once more (np.linalg.inv of the gathered blocks, the edits and products in the host function's
    order): what setupVankaFacesPreconditioner returned before the device path existed, to the bit on the same LAPACK."""
    Acc = S.gather(A, n, ip)
    cells, bs, _ = Acc.shape
    pair = isinstance(w, tuple)
    W = np.full(bs, float(w[0]) if pair else float(w))
    if pair and ip:
        W[-1] = float(w[1])
    lead = np.arange(bs - 1)
    if vtype == V.FULL_VANKA_RB and not pair:
        dg = Acc[:, lead, lead].copy()
        Acc[:, :bs - 1, :bs - 1] = 0.0
        Acc[:, lead, lead] = dg
        Minv = float(w) * np.linalg.inv(Acc)
    elif vtype == V.FULL_VANKA_RB:
        Minv = W[None, :, None] * np.linalg.inv(Acc)
    elif vtype == V.ECON_VANKA_RB:
        dg = Acc[:, lead, lead] / float(w)
        Acc[:, :bs - 1, :bs - 1] = 0.0
        Acc[:, lead, lead] = dg
        Minv = np.linalg.inv(Acc)
    else:
        t = np.full((cells, bs), 0.5)
        for c in range(cells):
            loc = V.cs2loc(c + 1, n)
            for d in range(len(n)):
                if loc[d] == 1:
                    t[c, 2 * d] = 1.0
                if loc[d] == n[d]:
                    t[c, 2 * d + 1] = 1.0
        t[:, -1] = 1.0 if ip else t[:, -1]
        Minv = (t * W[None, :])[:, :, None] * np.linalg.inv(Acc)
    return np.asfortranarray(np.conj(Minv).reshape(cells, bs * bs).T.astype(np.complex64 if np.iscomplexobj(Minv) else np.float32))


def test_host_path_is_untouched(mg):
    """device=False (and no device argument) give the bits the host path gave before the device path existed."""
    n, ip = [3, 2, 2], True
    A = S.operator(n, ip, True)
    for vtype, w in S.VARIANTS:
        a = mg.setupVankaFacesPreconditioner(A, np.asarray(n), w, ip, vtype)
        b = mg.setupVankaFacesPreconditioner(A, np.asarray(n), w, ip, vtype, device=False)
        assert a.dtype == np.complex64 and a.flags.f_contiguous and a.shape == (49, 12)
        assert a.tobytes(order="F") == b.tobytes(order="F")
        assert a.tobytes(order="F") == _host_expected(A, n, w, ip, vtype).tobytes(order="F")
    # FULL_VANKA_LEX blocks are still set up on the host (the device refuses the type)
    lex = mg.setupVankaFacesPreconditioner(A, np.asarray(n), 0.6, ip, V.FULL_VANKA_LEX)
    assert np.array_equal(lex, mg.setupVankaFacesPreconditioner(A, np.asarray(n), 0.6, ip, V.FULL_VANKA_RB))
    with pytest.raises(TypeError):
        mg.setupVankaFacesPreconditioner(A, np.asarray(n), (0.6, 0.4), ip, V.ECON_VANKA_RB)
