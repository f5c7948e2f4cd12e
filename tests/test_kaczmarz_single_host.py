"""Float32 / ComplexF32 hybrid Kaczmarz on the CPU (applyHybridKaczmarz_FP32_INT64 / _CFP32_INT64, deps/src/parRelax.h:7-43;
parRelax.jl:61-79): the mixed-precision restatement of tests/kaczmarz_single_cases.py against the reference's own binary (or
its stored outputs), the finding that an all-single restatement is NOT the binary, the single invDiag, the opt-in rules, the
type refusals before the device and the C ABI's argument checks.  The HIP kernel: tests/test_kaczmarz_single_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import kaczmarz_single_cases as K
from complex_cases import helmholtz

MG_OK, MG_ERR_INVALID, MG_ERR_HIP, MG_ERR_STATE, MG_ERR_UNSUPPORTED = 0, 1, 2, 3, 4


@pytest.mark.parametrize("name,tname", K.PAIRS)
def test_restatement_equals_reference_binary(mg, name, tname):
    """The restatement does the binary's operations with the binary's roundings (numCores = 1): bit for bit."""
    A, _, Arr, invD, b, x0 = K.case_inputs(mg, name, tname)
    x_ref = K.reference_output(mg, name, tname)
    assert x_ref.dtype == K.TYPES[tname] and np.isfinite(x_ref).all() and not np.array_equal(x_ref, x0)
    x = K.restate_apply_single(A, Arr, x0.copy(order="F"), b, invD, K.CASES[name][3])
    assert np.array_equal(x, x_ref)


@pytest.mark.parametrize("tname", list(K.TYPES))
def test_all_single_first_statement_is_not_the_binary(mg, tname):
    """`inner -= conj(valA)*x` done in single differs from the binary in the last bits on the long rows of `awkward`: the
    reference's conj() is the double one, which is why the device kernel mixes precisions."""
    A, _, Arr, invD, b, x0 = K.case_inputs(mg, "awkward", tname)
    x_ref = K.reference_output(mg, "awkward", tname)
    x = K.restate_apply_single(A, Arr, x0.copy(order="F"), b, invD, K.CASES["awkward"][3], first_statement_in_single=True)
    assert not np.array_equal(x, x_ref)
    d = np.abs(x.astype(np.complex128) - x_ref.astype(np.complex128)).max()
    print(f"all-single first statement, awkward {tname}: max abs difference {d:.3e}")
    assert d < 1e-4 * np.abs(x_ref).max()           # the last bits, not another method


@pytest.mark.parametrize("name,tname", [p for p in K.PAIRS if p[0] != "awkward"])
def test_single_invdiag(mg, name, tname):
    from oracle import mg_oracle as orc
    A, mesh, Arr, invD, _, _ = K.case_inputs(mg, name, tname)
    _, domains, _, numit = K.CASES[name]
    VAL = K.TYPES[tname]
    hk = mg.getHybridKaczmarz(VAL, np.int64, A, mesh, domains, mg.getNodalIndicesOfCell, K.OMEGA, 4, numit, singleValues=True)
    assert hk.is_single and hk.is_complex == (tname == "CFP32") and hk.VAL is VAL
    assert hk.invDiag.dtype == VAL and np.array_equal(hk.invDiag, invD)
    assert np.all(np.imag(hk.invDiag) == 0.0)
    cells = K.CASES[name][0]
    assert np.array_equal(hk.ArrIdxs, orc.getIndicesOfCellsArray(cells, [0] * len(cells), domains))
    assert np.array_equal(hk.ArrIdxs, Arr)
    # the single value is the double formula's to single accuracy: positive terms, each with at most two roundings of its
    # own and one per addition of the row (at most m of relative size 2^-24 in all), one more for the final rounding
    d = orc.hybrid_kaczmarz_invdiag(abs(A.astype(np.complex128)), K.OMEGA)
    m = int(np.diff(A.indptr).max()) + 3
    assert np.all(np.abs(hk.invDiag.real - d) <= 1.01 * m * 2.0 ** -24 * d)
    # a real operator handed to a ComplexF32 param is cast; a complex one to a Float32 param is refused
    if tname == "FP32":
        hc = mg.getHybridKaczmarz(np.complex64, np.int64, A, mesh, domains, mg.getNodalIndicesOfCell, K.OMEGA, 4, 1, singleValues=True)
        assert hc.invDiag.dtype == np.complex64 and np.array_equal(hc.invDiag.real, hk.invDiag)
    else:
        with pytest.raises(TypeError):
            mg.getHybridKaczmarz(np.float32, np.int64, A, mesh, domains, mg.getNodalIndicesOfCell, K.OMEGA, 4, 1, singleValues=True)


def test_opt_in_rules(mg):
    get, idx = mg.getHybridKaczmarz, mg.getNodalIndicesOfCell
    A, mesh = helmholtz(mg, [8, 8])
    # without the keyword nothing changes: Float64 for np.float32, TypeError for np.complex64 (both forms)
    p = get(np.float32, np.int64, [2, 2], idx, 0.8, 1, 1)
    assert not p.is_single and not p.is_complex and p.VAL is np.float64
    p = get(np.float32, np.int64, A.real.tocsr(), mesh, [2, 2], idx, 0.8, 1, 1)
    assert not p.is_single and p.invDiag.dtype == np.float64
    for args in [([2, 2], idx, 0.8, 1, 1), (A, mesh, [2, 2], idx, 0.8, 1, 1)]:
        with pytest.raises(TypeError):
            get(np.complex64, np.int64, *args)
        assert not get(np.complex128, np.int64, *args).is_single
        assert not get(np.complex128, np.int64, *args, singleValues=False).is_single
    # with it: a single param from a single VAL, TypeError from a double one (both forms)
    for VAL, cx in [(np.float32, False), (np.complex64, True)]:
        p = get(VAL, np.int64, [2, 2], idx, 0.8, 1, 1, singleValues=True)
        assert p.is_single and p.is_complex == cx and p.VAL is VAL and p.invDiag is None
    p = get(np.complex64, np.int64, A.astype(np.complex64), mesh, [2, 2], idx, 0.8, 1, 1, singleValues=True)
    assert p.is_single and p.is_complex and p.invDiag.dtype == np.complex64
    for VAL in (np.float64, np.complex128):
        for args in [([2, 2], idx, 0.8, 1, 1), (A, mesh, [2, 2], idx, 0.8, 1, 1)]:
            with pytest.raises(TypeError):
                get(VAL, np.int64, *args, singleValues=True)
    import inspect
    assert inspect.signature(get).parameters["singleValues"].kind is inspect.Parameter.KEYWORD_ONLY
    # the struct: the field comes last, the positional form keeps working and stays double
    arr = np.zeros((1, 1), np.uint32)
    inv = np.ones(4)
    assert not mg.hybridKaczmarz([1, 1], inv, 1, 0.8, arr, None, 1, idx).is_single
    assert mg.hybridKaczmarz([1, 1], inv + 0j, 1, 0.8, arr, None, 1, idx).VAL is np.complex128
    s = mg.hybridKaczmarz([1, 1], inv.astype(np.complex64), 1, 0.8, arr, None, 1, idx, singleValues=True)
    assert s.is_single and s.is_complex and s.VAL is np.complex64
    s = mg.hybridKaczmarz([1, 1], inv.astype(np.float32), 1, 0.8, arr, None, 1, idx, singleValues=True)
    assert s.is_single and not s.is_complex and s.VAL is np.float32
    with pytest.raises(TypeError):
        mg.hybridKaczmarz([1, 1], inv, 1, 0.8, arr, None, 1, idx, VAL=np.float64, singleValues=True)
    import dataclasses
    assert [f.name for f in dataclasses.fields(mg.hybridKaczmarz)][-1] == "singleValues"


def test_type_mismatch_raises_before_the_device(mg, monkeypatch):
    """A single param takes AT, r and x of exactly its dtype; everything else raises TypeError before any device call."""
    def no_device(*a, **k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(mg.device, "load_library", no_device)
    A, mesh = helmholtz(mg, [8, 8])
    n = A.shape[0]
    idx = mg.getNodalIndicesOfCell
    Ac, Ar = A.astype(np.complex64).tocsr(), A.real.astype(np.float32).tocsr()
    hc = mg.getHybridKaczmarz(np.complex64, np.int64, Ac, mesh, [2, 2], idx, 0.8, 1, 2, singleValues=True)
    hr = mg.getHybridKaczmarz(np.float32, np.int64, Ar, mesh, [2, 2], idx, 0.8, 1, 2, singleValues=True)
    hd = mg.getHybridKaczmarz(np.float64, np.int64, A.real.tocsr(), mesh, [2, 2], idx, 0.8, 1, 2)
    hz = mg.getHybridKaczmarz(np.complex128, np.int64, A, mesh, [2, 2], idx, 0.8, 1, 2)
    zc, zr = np.zeros(n, np.complex64), np.zeros(n, np.float32)
    bc, br = np.ones(n, np.complex64), np.ones(n, np.float32)
    w = lambda a: a.astype(np.complex128 if a.dtype.kind == "c" else np.float64)
    for args in [(hc, Ar, bc, zc), (hc, Ac, br, zc), (hc, Ac, bc, zr),                  # a real array on a ComplexF32 param
                 (hc, A, bc, zc), (hc, Ac, w(bc), zc), (hc, Ac, bc, w(zc)),             # a double array on a ComplexF32 param
                 (hr, Ac, br, zr), (hr, Ar, bc, zr), (hr, Ar, br, zc),                  # a complex array on a Float32 param
                 (hr, w(Ar), br, zr), (hr, Ar, w(br), zr), (hr, Ar, br, w(zr)),         # a double array on a Float32 param
                 (hz, Ac, w(bc), w(zc)), (hz, A, bc, w(zc)), (hz, A, w(bc), zc),        # a single array on a ComplexF64 param
                 (hd, Ac, w(br), w(zr)), (hd, w(Ar), bc, w(zr)), (hd, w(Ar), w(br), zc)]:
        with pytest.raises(TypeError):
            mg.applyHybridKaczmarz(*args)
    for p, M in [(hc, Ar), (hc, A), (hr, Ac), (hr, w(Ar))]:
        with pytest.raises(TypeError):
            mg.getHybridKaczmarzPrecond(p, M, 1)


@pytest.mark.parametrize("tname", list(K.TYPES))
def test_cabi_create_validates_like_cfp64(mg, built, tname):
    """The single entry points check their arguments as the CFP64 ones do (the same codes); without a GPU create fails
    loudly (no fallback) and leaves a null handle."""
    import torch
    lib = mg.device.load_library()
    A64, mesh = helmholtz(mg, [6, 6])
    A = K.cast_operator(A64, tname)
    n = A.shape[0]
    cp = np.ascontiguousarray(A.indptr, dtype=np.int64) + 1
    rv = np.ascontiguousarray(A.indices, dtype=np.int64) + 1
    nz = np.ascontiguousarray(np.conj(A.data))
    inv = K.invdiag_single(A, 0.8)
    arr = np.asfortranarray(mg.getIndicesOfCellsArray(mesh, [0, 0], [2, 2]), dtype=np.uint32)
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_longlong))
    F = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    U = arr.ctypes.data_as(C.POINTER(C.c_uint))
    h = C.c_void_p()
    create = getattr(lib, f"mg_kaczmarz_create_{tname}_INT64")
    apply = getattr(lib, f"mg_kaczmarz_apply_{tname}")
    assert create(0, n, P(cp), F(nz), P(rv), arr.shape[1], arr.shape[0], U, F(inv), None) == MG_ERR_INVALID
    assert create(0, n, P(cp), None, P(rv), arr.shape[1], arr.shape[0], U, F(inv), C.byref(h)) == MG_ERR_INVALID
    bad = cp.copy()
    bad[0] = 0                                        # not a 1-based pointer array
    assert create(0, n, P(bad), F(nz), P(rv), arr.shape[1], arr.shape[0], U, F(inv), C.byref(h)) == MG_ERR_INVALID
    assert create(0, 1 << 31, P(cp), F(nz), P(rv), arr.shape[1], arr.shape[0], U, F(inv), C.byref(h)) == MG_ERR_UNSUPPORTED
    x = np.zeros(n, K.TYPES[tname])
    assert apply(None, F(x), F(x), 1, 1, 1) == MG_ERR_INVALID
    assert getattr(lib, f"mg_kaczmarz_apply_dev_{tname}")(None, 0, 0, 1, 1, 1) == MG_ERR_INVALID
    rc = create(0, n, P(cp), F(nz), P(rv), arr.shape[1], arr.shape[0], U, F(inv), C.byref(h))
    if torch.cuda.is_available():
        assert rc == MG_OK
        lib.mg_kaczmarz_destroy(h)
    else:
        assert rc == MG_ERR_HIP and not h.value
