"""ComplexF64 hybrid Kaczmarz (applyHybridKaczmarz_CFP64_INT64, deps/src/parRelax.h:7-43; parRelax.jl:71-74): the literal
restatement of tests/kaczmarz_complex_cases.py against the reference's own binary, the complex invDiag, the type refusals
and the C ABI's argument checks on the CPU; the HIP kernel hybrid_kaczmarz_c through mg_kaczmarz_*_CFP64 on the GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import kaczmarz_complex_cases as K
from complex_cases import complex_rhs, helmholtz
from oracle import mg_oracle as orc

MG_OK, MG_ERR_INVALID, MG_ERR_HIP, MG_ERR_STATE = 0, 1, 2, 3


def _param(mg, name, VAL=np.complex128, sequential=True):
    A, mesh, Arr, invD, b = K.case_inputs(mg, name)
    _, domains, _, numit = K.CASES[name]
    hk = mg.getHybridKaczmarz(VAL, np.int64, A, mesh, domains, mg.getNodalIndicesOfCell, K.OMEGA, 4, numit)
    hk.sequential = sequential
    return hk, A, Arr, invD, b


# ---- CPU -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.CASES))
def test_restatement_equals_reference_binary(mg, name):
    """The restatement does the binary's operations in the binary's order (numCores = 1): bit for bit."""
    A, _, Arr, invD, b = K.case_inputs(mg, name)
    numit = K.CASES[name][3]
    x_ref = K.reference_output(name, lambda: K.run_reference_case(mg, name))
    x = K.restate_apply(A, Arr, np.zeros_like(b, order="F"), b, invD, numit)
    assert np.array_equal(x, x_ref)
    assert np.linalg.norm(A @ x - b) < np.linalg.norm(b)


@pytest.mark.parametrize("name", list(K.CASES))
def test_complex_invdiag(mg, name):
    hk, A, Arr, invD, _ = _param(mg, name)
    assert hk.is_complex and hk.invDiag.dtype == np.complex128
    assert np.array_equal(hk.invDiag, invD) and np.all(hk.invDiag.imag == 0.0)
    assert np.array_equal(hk.ArrIdxs, Arr)
    # a real operator: the Float64 invDiag is what it always was; the ComplexF64 one holds the same values
    R = K.case_inputs(mg, name)[0].real.tocsr()
    _, mesh = helmholtz(mg, K.CASES[name][0])
    hr = mg.getHybridKaczmarz(np.float64, np.int64, R, mesh, K.CASES[name][1], mg.getNodalIndicesOfCell, K.OMEGA, 4, 1)
    assert not hr.is_complex and hr.invDiag.dtype == np.float64
    assert np.array_equal(hr.invDiag, orc.hybrid_kaczmarz_invdiag(R, K.OMEGA))
    hc = mg.getHybridKaczmarz(np.complex128, np.int64, R, mesh, K.CASES[name][1], mg.getNodalIndicesOfCell, K.OMEGA, 4, 1)
    assert hc.invDiag.dtype == np.complex128 and np.array_equal(hc.invDiag.real, hr.invDiag)


def test_param_value_type(mg):
    A, mesh = helmholtz(mg, [8, 8])
    inv = K.invdiag(A, 0.8)
    arr = np.zeros((1, 1), np.uint32)
    assert mg.hybridKaczmarz([1, 1], inv, 1, 0.8, arr, None, 1, mg.getNodalIndicesOfCell).is_complex          # positional form
    assert not mg.hybridKaczmarz([1, 1], inv.real, 1, 0.8, arr, None, 1, mg.getNodalIndicesOfCell).is_complex
    assert mg.getHybridKaczmarz(np.complex128, np.int64, [2, 2], mg.getNodalIndicesOfCell, 0.8, 1, 1).is_complex
    with pytest.raises(TypeError):
        mg.getHybridKaczmarz(np.complex64, np.int64, [2, 2], mg.getNodalIndicesOfCell, 0.8, 1, 1)


def test_type_mismatch_raises_before_the_device(mg, monkeypatch):
    """A Float64 param refuses every complex array and a ComplexF64 param every other one, before any device call."""
    def no_device(*a, **k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(mg.device, "load_library", no_device)
    A, mesh = helmholtz(mg, [8, 8])
    n = A.shape[0]
    hc = mg.getHybridKaczmarz(np.complex128, np.int64, A, mesh, [2, 2], mg.getNodalIndicesOfCell, 0.8, 1, 2)
    hr = mg.getHybridKaczmarz(np.float64, np.int64, A.real.tocsr(), mesh, [2, 2], mg.getNodalIndicesOfCell, 0.8, 1, 2)
    zc, zr = np.zeros(n, np.complex128), np.zeros(n)
    bc, br = complex_rhs(n), np.ones(n)
    R = A.real.tocsr()
    for args in [(hr, A, br, zr), (hr, R, bc, zr), (hr, R, br, zc),                                  # complex into Float64
                 (hc, R, bc, zc), (hc, A, br, zc), (hc, A, bc, zr), (hc, A, bc.astype(np.complex64), zc),
                 (hc, A.astype(np.complex64), bc, zc), (hc, A, bc, zc.astype(np.complex64))]:
        with pytest.raises(TypeError):
            mg.applyHybridKaczmarz(*args)
    with pytest.raises(TypeError):
        mg.getHybridKaczmarzPrecond(hr, A, 1)
    with pytest.raises(TypeError):
        mg.getHybridKaczmarzPrecond(hc, R, 1)


def test_cabi_create_validates_like_fp64(mg, built):
    """The CFP64 entry points check their arguments as the FP64 ones do; without a GPU create fails loudly (no fallback)."""
    import torch
    lib = mg.device.load_library()
    A, mesh = helmholtz(mg, [6, 6])
    n = A.shape[0]
    cp = np.ascontiguousarray(A.indptr, dtype=np.int64) + 1
    rv = np.ascontiguousarray(A.indices, dtype=np.int64) + 1
    nz = np.ascontiguousarray(np.conj(A.data))
    inv = K.invdiag(A, 0.8)
    arr = np.asfortranarray(mg.getIndicesOfCellsArray(mesh, [0, 0], [2, 2]), dtype=np.uint32)
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_longlong))
    D = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    U = arr.ctypes.data_as(C.POINTER(C.c_uint))
    h = C.c_void_p()
    create = lib.mg_kaczmarz_create_CFP64_INT64
    assert create(0, n, P(cp), D(nz), P(rv), arr.shape[1], arr.shape[0], U, D(inv), None) == MG_ERR_INVALID
    assert create(0, n, P(cp), None, P(rv), arr.shape[1], arr.shape[0], U, D(inv), C.byref(h)) == MG_ERR_INVALID
    bad = cp.copy()
    bad[0] = 0                                        # not a 1-based pointer array
    assert create(0, n, P(bad), D(nz), P(rv), arr.shape[1], arr.shape[0], U, D(inv), C.byref(h)) == MG_ERR_INVALID
    assert create(0, 1 << 31, P(cp), D(nz), P(rv), arr.shape[1], arr.shape[0], U, D(inv), C.byref(h)) == 4   # UNSUPPORTED
    x = np.zeros(n, np.complex128)
    assert lib.mg_kaczmarz_apply_CFP64(None, D(x), D(x), 1, 1, 1) == MG_ERR_INVALID
    rc = create(0, n, P(cp), D(nz), P(rv), arr.shape[1], arr.shape[0], U, D(inv), C.byref(h))
    if torch.cuda.is_available():
        assert rc == MG_OK
        lib.mg_kaczmarz_destroy(h)
    else:
        assert rc == MG_ERR_HIP and not h.value


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(K.CASES))
def test_device_sequential_equals_reference_binary(mg, built, name):
    """One wavefront walking the sub-domains in order: the reference binary with numCores = 1 bit for bit (nrhs 1, 2, 3)."""
    hk, A, Arr, invD, b = _param(mg, name)
    assert np.array_equal(hk.invDiag, invD) and np.array_equal(hk.ArrIdxs, Arr)
    x = np.zeros_like(b, order="F")
    assert mg.applyHybridKaczmarz(hk, A, b, x) is x
    assert np.array_equal(x, K.reference_output(name, lambda: K.run_reference_case(mg, name)))
    # a second call on the same param reuses the upload and sweeps on from the x it is given
    x2 = x.copy(order="F")
    mg.applyHybridKaczmarz(hk, A, b, x2)
    assert np.array_equal(x2, K.restate_apply(A, Arr, x.copy(order="F"), b, invD, K.CASES[name][3]))
    hk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nrhs", [1, 2])
def test_device_parallel_block_diagonal_exact(mg, built, nrhs):
    """One wavefront per sub-domain on an operator whose sub-domains do not couple: no races, so exact against the
    restatement.  Rows within each sub-domain are listed in a random order."""
    A1, _ = K.helmholtz_unsym(mg, [12, 12], seed=3)
    n1 = A1.shape[0]
    A = sp.block_diag([A1] * 4, format="csr")
    A.sort_indices()
    rng = np.random.default_rng(2)
    arr = np.zeros((n1, 4), dtype=np.uint32, order="F")
    for d in range(4):
        arr[:, d] = rng.permutation(n1) + 1 + d * n1
    invD = K.invdiag(A, K.OMEGA)
    hk = mg.hybridKaczmarz([4, 1], invD, 4, K.OMEGA, arr, None, 3, mg.getNodalIndicesOfCell)
    assert hk.is_complex and not hk.sequential
    b = K.complex_block(A, nrhs, 9)
    x = np.zeros_like(b, order="F")
    mg.applyHybridKaczmarz(hk, A, b, x)
    assert np.array_equal(x, K.restate_apply(A, arr, np.zeros_like(b, order="F"), b, invD, 3))
    hk.close()


@pytest.mark.gpu
def test_device_preconditioner_for_gmres(mg, built):
    """Sequential sweeps as scipy gmres's preconditioner on a 2-D Helmholtz operator (getHybridKaczmarzPrecond): fewer
    iterations than without one, and the iterate of the same gmres run with the restatement as preconditioner.  Then the
    parallel schedule: one application's residual within 10x of the reference binary's at 4 threads, where it is built."""
    A, mesh = helmholtz(mg, [32, 32])
    b = complex_rhs(A.shape[0], 3)
    numit, omega = 10, 1.0
    hk = mg.getHybridKaczmarz(np.complex128, np.int64, A, mesh, [4, 4], mg.getNodalIndicesOfCell, omega, 4, numit)
    hk.sequential = True
    prec = mg.getHybridKaczmarzPrecond(hk, A, 1)

    def gmres(M):
        count = [0]
        x, info = spla.gmres(A, b, rtol=1e-8, restart=30, maxiter=40, M=M, callback_type="pr_norm",
                             callback=lambda r: count.__setitem__(0, count[0] + 1))
        assert info == 0
        return x, count[0]

    op = lambda f: spla.LinearOperator(A.shape, matvec=f, dtype=np.complex128)
    x_plain, it_plain = gmres(None)
    x_dev, it_dev = gmres(op(lambda r: prec(np.asarray(r).ravel()).copy()))
    x_res, it_res = gmres(op(lambda r: K.restate_apply(A, hk.ArrIdxs, np.zeros(A.shape[0], np.complex128),
                                                        np.asarray(r).ravel(), hk.invDiag, numit)))
    assert it_dev < it_plain
    assert it_dev == it_res and np.abs(x_dev - x_res).max() <= 1e-10 * np.abs(x_res).max()
    hk.close()

    name = "kaczmarz_c_64x64_d4x4_nrhs2_it5"
    hp, A, Arr, invD, b = _param(mg, name, sequential=False)
    x = np.zeros_like(b, order="F")
    mg.applyHybridKaczmarz(hp, A, b, x)
    res_dev = np.linalg.norm(A @ x - b)
    assert res_dev < np.linalg.norm(b)
    if os.path.exists(K.REF):
        xr = K.ref_apply(A, Arr, np.zeros_like(b, order="F"), b, invD, K.CASES[name][3], 4)
        assert res_dev < 10.0 * np.linalg.norm(A @ xr - b) + 1e-12
    hp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nrhs", [1, 3])
def test_device_entry_on_torch_tensors_equals_host_entry(mg, built, nrhs):
    import torch
    from multigrid_jl_amd import par_relax
    name = "kaczmarz_c_64x64_d4x4_nrhs2_it5"
    hk, A, _, _, _ = _param(mg, name)
    b = K.complex_block(A, nrhs, 4)
    x0 = K.complex_block(A, nrhs, 5)                  # a non-zero start
    x_host = x0.copy(order="F")
    mg.applyHybridKaczmarz(hk, A, b, x_host)
    h = par_relax._device_handle(hk, A)
    n = A.shape[0]
    # an n x nrhs column-major block is an (nrhs, n) row-major tensor
    xt = torch.from_numpy(np.ascontiguousarray(x0.reshape(n, nrhs, order="F").T)).cuda()
    bt = torch.from_numpy(np.ascontiguousarray(b.reshape(n, nrhs, order="F").T)).cuda()
    torch.cuda.synchronize()
    lib = mg.device.load_library()
    assert lib.mg_kaczmarz_apply_dev_CFP64(h, xt.data_ptr(), bt.data_ptr(), nrhs, hk.numit, 1) == MG_OK
    x_dev = xt.cpu().numpy().T.reshape(x0.shape, order="F")
    assert np.array_equal(x_dev, x_host)
    hk.close()


@pytest.mark.gpu
def test_mixed_value_types_refused_handle_survives(mg, built):
    """An FP64 apply on a CFP64 handle and a CFP64 apply on an FP64 handle return MG_ERR_STATE; both handles work after."""
    import torch
    from multigrid_jl_amd import par_relax
    lib = mg.device.load_library()
    name = "kaczmarz_c_30x20_d3x2_nrhs3_it2"
    hc, A, Arr, invD, b = _param(mg, name)
    R = A.real.tocsr()
    _, mesh = helmholtz(mg, K.CASES[name][0])
    hr = mg.getHybridKaczmarz(np.float64, np.int64, R, mesh, K.CASES[name][1], mg.getNodalIndicesOfCell, K.OMEGA, 4, 2)
    hr.sequential = True
    n, nrhs = A.shape[0], b.shape[1]
    h_c, h_r = par_relax._device_handle(hc, A), par_relax._device_handle(hr, R)
    # buffers large enough for either value type, so a refusal that failed could not reach past them
    xh = np.zeros(2 * n * nrhs)
    bh = np.ones(2 * n * nrhs)
    xt = torch.zeros(2 * n * nrhs, dtype=torch.float64, device="cuda")
    bt = torch.ones(2 * n * nrhs, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.mg_kaczmarz_apply_FP64(h_c, dp(xh), dp(bh), nrhs, 1, 1) == MG_ERR_STATE
    assert lib.mg_kaczmarz_apply_dev_FP64(h_c, xt.data_ptr(), bt.data_ptr(), nrhs, 1, 1) == MG_ERR_STATE
    assert lib.mg_kaczmarz_apply_CFP64(h_r, dp(xh), dp(bh), nrhs, 1, 1) == MG_ERR_STATE
    assert lib.mg_kaczmarz_apply_dev_CFP64(h_r, xt.data_ptr(), bt.data_ptr(), 1, 1, 1) == MG_ERR_STATE
    assert np.all(xh == 0.0)
    # both handles still sweep correctly
    x = np.zeros_like(b, order="F")
    mg.applyHybridKaczmarz(hc, A, b, x)
    assert np.array_equal(x, K.restate_apply(A, Arr, np.zeros_like(b, order="F"), b, invD, 2))
    br = np.asfortranarray(b.real)
    xr = np.zeros_like(br, order="F")
    mg.applyHybridKaczmarz(hr, R, br, xr)
    xo = np.zeros_like(br, order="F")
    orc.applyHybridKaczmarz(R, hr.ArrIdxs, xo, br, hr.invDiag, 2)
    assert np.array_equal(xr, xo)
    hc.close()
    hr.close()
