"""Float32 / ComplexF32 hybrid Kaczmarz on the GPU: the HIP kernel hybrid_kaczmarz_s<float> / <f2_t> through
mg_kaczmarz_*_FP32 / _CFP32 and the Python entry points, against the reference binary's outputs and the mixed-precision
restatement of tests/kaczmarz_single_cases.py (whose CPU checks are in tests/test_kaczmarz_single_host.py)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import kaczmarz_single_cases as K
from kaczmarz_complex_cases import helmholtz_unsym

pytestmark = pytest.mark.gpu

MG_OK, MG_ERR_INVALID, MG_ERR_HIP, MG_ERR_STATE = 0, 1, 2, 3
TORCH = {"FP32": "float32", "CFP32": "complex64"}


def _param(mg, name, tname, sequential=True):
    """The single param of a (case, type) pair: through getHybridKaczmarz on the grids, the struct itself for `awkward`."""
    A, mesh, Arr, invD, b, x0 = K.case_inputs(mg, name, tname)
    _, domains, _, numit = K.CASES[name]
    if mesh is None:
        hk = mg.hybridKaczmarz([Arr.shape[1], 1], invD, Arr.shape[1], K.OMEGA, Arr, None, numit, mg.getNodalIndicesOfCell,
                               singleValues=True)
    else:
        hk = mg.getHybridKaczmarz(K.TYPES[tname], np.int64, A, mesh, domains, mg.getNodalIndicesOfCell, K.OMEGA, 4, numit,
                                  singleValues=True)
    assert hk.is_single and hk.VAL is K.TYPES[tname]
    hk.sequential = sequential
    return hk, A, Arr, invD, b, x0


@pytest.mark.parametrize("name,tname", K.PAIRS)
def test_device_sequential_equals_reference_binary(mg, built, name, tname):
    """One wavefront walking the sub-domains in order, from a non-zero x: the reference binary with numCores = 1 bit for
    bit.  A second call reuses the upload and sweeps on from the x it is given."""
    hk, A, Arr, invD, b, x0 = _param(mg, name, tname)
    assert np.array_equal(hk.invDiag, invD) and np.array_equal(hk.ArrIdxs, Arr)
    numit = K.CASES[name][3]
    x = x0.copy(order="F")
    assert mg.applyHybridKaczmarz(hk, A, b, x) is x
    assert x.dtype == K.TYPES[tname]
    assert np.array_equal(x, K.reference_output(mg, name, tname))
    h = hk._handle
    x2 = x.copy(order="F")
    mg.applyHybridKaczmarz(hk, A, b, x2)
    assert hk._handle is h
    assert np.array_equal(x2, K.restate_apply_single(A, Arr, x.copy(order="F"), b, invD, numit))
    hk.close()


@pytest.mark.parametrize("tname", list(K.TYPES))
@pytest.mark.parametrize("nrhs", [1, 2])
def test_device_parallel_block_diagonal_exact(mg, built, nrhs, tname):
    """One wavefront per sub-domain on an operator whose sub-domains do not couple: no races, so exact against the
    restatement.  Rows within each sub-domain are listed in a random order."""
    A1, _ = helmholtz_unsym(mg, [10, 10], seed=3)
    n1 = A1.shape[0]
    A = K.cast_operator(sp.block_diag([A1] * 4, format="csr"), tname)
    rng = np.random.default_rng(2)
    arr = np.zeros((n1, 4), dtype=np.uint32, order="F")
    for d in range(4):
        arr[:, d] = rng.permutation(n1) + 1 + d * n1
    invD = K.invdiag_single(A, K.OMEGA)
    hk = mg.hybridKaczmarz([4, 1], invD, 4, K.OMEGA, arr, None, 3, mg.getNodalIndicesOfCell, singleValues=True)
    assert hk.is_single and not hk.sequential
    b = K.single_block(A.shape[0], nrhs, 9, tname, 0.05)
    x0 = K.single_block(A.shape[0], nrhs, 10, tname, 0.05)
    x = x0.copy(order="F")
    mg.applyHybridKaczmarz(hk, A, b, x)
    assert np.array_equal(x, K.restate_apply_single(A, arr, x0.copy(order="F"), b, invD, 3))
    hk.close()


@pytest.mark.parametrize("tname", list(K.TYPES))
def test_device_parallel_coupled_reduces_residual(mg, built, tname):
    """One wavefront per sub-domain on grid2d, where the sub-domains couple and race: the sweeps still reduce the residual
    from x = 0 (what the ComplexF64 test asserts of its parallel schedule)."""
    hk, A, _, _, b, x0 = _param(mg, "grid2d", tname, sequential=False)
    x = np.zeros_like(x0, order="F")
    mg.applyHybridKaczmarz(hk, A, b, x)
    A64, x64, b64 = A.astype(np.complex128), x.astype(np.complex128), b.astype(np.complex128)
    assert np.isfinite(x).all() and np.linalg.norm(A64 @ x64 - b64) < np.linalg.norm(b64)
    hk.close()


@pytest.mark.parametrize("tname", list(K.TYPES))
def test_device_preconditioner_closure(mg, built, tname):
    """getHybridKaczmarzPrecond on grid3d, sequential: r -> the restatement's vector from x = 0, bit for bit, in one buffer
    that the closure reuses."""
    hk, A, Arr, invD, b, _ = _param(mg, "grid3d", tname)
    prec = mg.getHybridKaczmarzPrecond(hk, A, 1)
    assert hk.precond is prec
    y = prec(b)
    assert y.dtype == K.TYPES[tname] and y.shape == b.shape
    want = K.restate_apply_single(A, Arr, np.zeros_like(b), b, invD, K.CASES["grid3d"][3])
    assert np.array_equal(y, want)
    b2 = K.single_block(A.shape[0], 1, 21, tname, 0.1)
    y2 = prec(b2)
    assert y2 is y
    assert np.array_equal(y2, K.restate_apply_single(A, Arr, np.zeros_like(b), b2, invD, K.CASES["grid3d"][3]))
    hk.close()


@pytest.mark.parametrize("tname", list(K.TYPES))
def test_device_entry_on_torch_tensors_equals_host_entry(mg, built, tname):
    """mg_kaczmarz_apply_dev_* on torch tensors (an n x nrhs column-major block is an (nrhs, n) row-major tensor) equals the
    host entry; a pointer that is not aligned to one value is MG_ERR_INVALID (nothing is launched)."""
    import torch
    from multigrid_jl_amd import par_relax
    hk, A, _, _, b, x0 = _param(mg, "grid2d", tname)
    n, nrhs = b.shape
    x_host = x0.copy(order="F")
    mg.applyHybridKaczmarz(hk, A, b, x_host)
    h = par_relax._device_handle(hk, A)
    dt = getattr(torch, TORCH[tname])
    # one spare value at the end: the misaligned views below stay inside the allocation
    xt = torch.zeros(nrhs * n + 1, dtype=dt, device="cuda")
    bt = torch.zeros(nrhs * n + 1, dtype=dt, device="cuda")
    xt[:nrhs * n] = torch.from_numpy(x0.T.copy(order="C")).reshape(-1).cuda()
    bt[:nrhs * n] = torch.from_numpy(b.T.copy(order="C")).reshape(-1).cuda()
    torch.cuda.synchronize()
    lib = mg.device.load_library()
    apply_dev = getattr(lib, f"mg_kaczmarz_apply_dev_{tname}")
    off = xt.element_size() // 2                       # 2 of 4 bytes, 4 of 8
    before = xt.cpu().numpy().copy()
    assert apply_dev(h, xt.data_ptr() + off, bt.data_ptr(), nrhs, hk.numit, 1) == MG_ERR_INVALID
    assert apply_dev(h, xt.data_ptr(), bt.data_ptr() + off, nrhs, hk.numit, 1) == MG_ERR_INVALID
    torch.cuda.synchronize()
    assert np.array_equal(xt.cpu().numpy(), before)
    assert apply_dev(h, xt.data_ptr(), bt.data_ptr(), nrhs, hk.numit, 1) == MG_OK
    x_dev = xt[:nrhs * n].cpu().numpy().reshape(nrhs, n).T
    assert np.array_equal(x_dev, x_host)
    hk.close()


def test_cross_type_applies_refused_handles_survive(mg, built):
    """Every apply entry on a handle of another value type returns MG_ERR_STATE and touches nothing: FP32 <-> CFP32,
    FP32 <-> FP64, CFP32 <-> CFP64 (host and device forms, buffers sized for the widest type); the handles sweep correctly
    afterwards."""
    import torch
    from multigrid_jl_amd import par_relax
    from oracle import mg_oracle as orc
    import kaczmarz_complex_cases as KC
    lib = mg.device.load_library()
    hs, As, Arr, invDs, bs, x0s = _param(mg, "grid2d", "FP32")
    hc, Ac, _, invDc, bc, x0c = _param(mg, "grid2d", "CFP32")
    cells, domains, nrhs, numit = K.CASES["grid2d"]
    A128, mesh = helmholtz_unsym(mg, cells)
    R64 = A128.real.tocsr()
    hd = mg.getHybridKaczmarz(np.float64, np.int64, R64, mesh, domains, mg.getNodalIndicesOfCell, K.OMEGA, 4, numit)
    hz = mg.getHybridKaczmarz(np.complex128, np.int64, A128, mesh, domains, mg.getNodalIndicesOfCell, K.OMEGA, 4, numit)
    hd.sequential = hz.sequential = True
    n = As.shape[0]
    handle = {"FP32": par_relax._device_handle(hs, As), "CFP32": par_relax._device_handle(hc, Ac),
              "FP64": par_relax._device_handle(hd, R64), "CFP64": par_relax._device_handle(hz, A128)}
    # 16 bytes per value: large enough for any of the four types, so a refusal that failed could not reach past them
    xh, bh = np.zeros(2 * n * nrhs), np.ones(2 * n * nrhs)
    xt = torch.zeros(2 * n * nrhs, dtype=torch.float64, device="cuda")
    bt = torch.ones(2 * n * nrhs, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ptr = lambda a, entry: a.ctypes.data_as(C.POINTER(C.c_float if entry.endswith("32") else C.c_double))
    for entry, other in [("FP32", "CFP32"), ("CFP32", "FP32"), ("FP32", "FP64"), ("FP64", "FP32"), ("CFP32", "CFP64"),
                         ("CFP64", "CFP32"), ("FP64", "CFP32"), ("CFP32", "FP64")]:
        host, dev = getattr(lib, f"mg_kaczmarz_apply_{entry}"), getattr(lib, f"mg_kaczmarz_apply_dev_{entry}")
        assert host(handle[other], ptr(xh, entry), ptr(bh, entry), nrhs, 1, 1) == MG_ERR_STATE, (entry, other)
        assert dev(handle[other], xt.data_ptr(), bt.data_ptr(), nrhs, 1, 1) == MG_ERR_STATE, (entry, other)
        assert entry in lib.mg_last_error().decode() and other in lib.mg_last_error().decode()
    torch.cuda.synchronize()
    assert np.all(xh == 0.0) and bool((xt == 0).all())
    # all four handles still sweep correctly
    for hk, A, invD, b, x0, tname in [(hs, As, invDs, bs, x0s, "FP32"), (hc, Ac, invDc, bc, x0c, "CFP32")]:
        x = x0.copy(order="F")
        mg.applyHybridKaczmarz(hk, A, b, x)
        assert np.array_equal(x, K.reference_output(mg, "grid2d", tname))
    b128 = KC.complex_block(A128, nrhs, 11)
    x = np.zeros_like(b128, order="F")
    mg.applyHybridKaczmarz(hz, A128, b128, x)
    assert np.array_equal(x, KC.restate_apply(A128, Arr, np.zeros_like(b128, order="F"), b128, hz.invDiag, numit))
    b64 = np.asfortranarray(b128.real)
    x, xo = np.zeros_like(b64, order="F"), np.zeros_like(b64, order="F")
    mg.applyHybridKaczmarz(hd, R64, b64, x)
    orc.applyHybridKaczmarz(R64, hd.ArrIdxs, xo, b64, hd.invDiag, numit)
    assert np.array_equal(x, xo)
    for hk in (hs, hc, hd, hz):
        hk.close()
