"""Host side of the Float32 / ComplexF32 Schwarz sweep (opt-in: getDomainDecompositionParam(..., singleValues=True)): the keyword
rules and refusals, the single factors setupDDSerial keeps, the mixed closure's dtypes, the new C ABI names with their argument
types, the fixture guard of tests/dd_single_cases.py, and the pins of the default paths.  No GPU needed: every refusal here is raised
before the device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import coarse_solver_cases as csc
import dd_cases
import dd_single_cases as dsc
from complex_cases import helmholtz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgvcycle.h")
_ll, _lp, _fp, _up, _vp = C.c_longlong, C.POINTER(C.c_longlong), C.POINTER(C.c_float), C.POINTER(C.c_uint), C.c_void_p
_create = [_ll, _ll, _lp, _lp, _fp, _ll, _lp, _up, _lp, C.POINTER(_vp)]
_factor = lambda ip: [_vp, _ll, _ll, _lp, ip, _fp, _lp, ip, _fp, ip, ip]
NEW = {"mg_dd_create_FP32_INT64": _create, "mg_dd_create_CFP32_INT64": _create,
       "mg_dd_set_factor_FP32_UINT32": _factor(_up), "mg_dd_set_factor_CFP32_UINT32": _factor(_up),
       "mg_dd_set_factor_CFP32_INT64": _factor(_lp),
       "mg_dd_apply_FP32": [_vp, _fp, _fp, _ll, _ll, _ll], "mg_dd_apply_CFP32": [_vp, _fp, _fp, _ll, _ll, _ll],
       "mg_dd_apply_dev_FP32": [_vp, _vp, _vp, _ll, _ll, _ll], "mg_dd_apply_dev_CFP32": [_vp, _vp, _vp, _ll, _ll, _ll],
       "mg_dd0_apply_FP32": [_vp, _fp, _fp, _ll, _ll], "mg_dd0_apply_CFP32": [_vp, _fp, _fp, _ll, _ll],
       "mg_dd0_apply_dev_FP32": [_vp, _vp, _vp, _ll, _ll], "mg_dd0_apply_dev_CFP32": [_vp, _vp, _vp, _ll, _ll]}


def _pjs(mg, VAL, IND=np.uint32):
    return mg.ParallelJuliaSolver.getParallelJuliaSolver(VAL, IND, singleFactors=True)


def _mesh(mg):
    return mg.getRegularMesh([0.0, 1.0, 0.0, 1.0], [8, 8])


def test_keyword_rules(mg):
    mesh = _mesh(mg)
    args = (np.int64, mesh, [2, 2], [1, 1], mg.getNodalIndicesOfCell)
    for VAL in (np.float32, np.complex64):
        with pytest.raises(TypeError):                                   # the default path: single values are refused as before
            mg.getDomainDecompositionParam(VAL, *args, None)
        p = mg.getDomainDecompositionParam(VAL, *args, _pjs(mg, VAL), singleValues=True)
        assert p.singleValues and p.is_single and np.dtype(p.VAL) == np.dtype(VAL) and p.is_complex == (VAL is np.complex64)
    for VAL in (np.float64, np.complex128):                              # the keyword with a double VAL (as getHybridKaczmarz)
        with pytest.raises(TypeError):
            mg.getDomainDecompositionParam(VAL, *args, None, singleValues=True)
        p = mg.getDomainDecompositionParam(VAL, *args, None)
        assert not p.singleValues and not p.is_single
    with pytest.raises(TypeError):                                       # keyword-only
        mg.getDomainDecompositionParam(np.float32, *args, None, True)
    with pytest.raises(TypeError):
        mg.getDomainDecompositionParam(np.float16, *args, None, singleValues=True)


def test_copy_solver_carries_the_keyword(mg):
    DD = mg.DomainDecomposition
    c = dsc.case(mg, "helmholtz2d_c32_t0")
    p = c.dd_param(mg)
    q = DD.copySolver(p)
    assert q.singleValues and np.dtype(q.VAL) == np.complex64 and DD.isempty(q) and not DD.isempty(p)
    assert q.Ainv is not p.Ainv and q.Ainv.singleFactors and np.dtype(q.Ainv.IND) == np.dtype(p.Ainv.IND)
    assert (q.numDomains, q.overlap) == (p.numDomains, p.overlap)
    d = DD.copySolver(dd_cases.dd_param(mg, *dd_cases.poisson(mg, [8, 8])[:2], [2, 2], [1, 1]))
    assert not d.singleValues and np.dtype(d.VAL) == np.float64


@pytest.mark.parametrize("name", ["poisson2d_f32", "helmholtz2d_c32_t0", "helmholtz2d_c32_t1", "uneven_f32"])
def test_setup_keeps_single_factors_of_a_double_factorisation(mg, name):
    """Every sub-domain's factors equal single_layout of a double splu of A[I, I] (the rounded operator widened back), bit for bit."""
    c = dsc.case(mg, name)
    p = c.dd_param(mg)
    assert len(p.PrecParams) == len(c.lists) == int(np.prod(c.boxes))
    for k, (prec, I, F) in enumerate(zip(p.PrecParams, c.lists, c.F)):
        s = prec.Ainv
        assert np.array_equal(p.GlobalIndices[k].astype(np.int64) - 1, I)
        assert s.singleFactors and s._handle is None
        assert s.L.dtype == s.U.dtype == np.dtype(c.VAL) and s.p.dtype == s.q.dtype == np.dtype(c.IND)
        assert np.array_equal(s.L.indptr + 1, F["Lp"]) and np.array_equal(s.U.indptr + 1, F["Up"])
        assert np.array_equal(s.L.indices + 1, F["Lc"]) and np.array_equal(s.U.indices + 1, F["Uc"])
        assert np.array_equal(s.L.data, F["Lv"]) and np.array_equal(s.U.data, F["Uv"])
        assert np.array_equal(s.p, F["p"]) and np.array_equal(s.q, F["q"])


def test_setup_refusals(mg):
    PJ = mg.ParallelJuliaSolver
    c = dsc.case(mg, "helmholtz2d_c32_t0")
    args = (np.int64, c.mesh, c.boxes, c.overlap, mg.getNodalIndicesOfCell)
    mk = lambda VAL, Ainv: mg.getDomainDecompositionParam(VAL, *args, Ainv, singleValues=True)
    with pytest.raises(NotImplementedError):                             # a double solver under a single param
        mg.setupDDSerial(c.A, mk(np.complex64, PJ.getParallelJuliaSolver(np.complex128, np.int64)))
    with pytest.raises(NotImplementedError):                             # a single solver of the other VAL
        mg.setupDDSerial(c.A, mk(np.complex64, _pjs(mg, np.float32)))
    with pytest.raises(TypeError):                                       # VAL matches, but not an opted-in single form
        mg.setupDDSerial(c.A, mk(np.complex64, PJ.parallelJuliaSolver(VAL=np.complex64, IND=np.int64)))
    for bad in (c.A.astype(np.complex128), c.A.real.astype(np.float32).tocsr()):   # A is not converted for the caller
        with pytest.raises(TypeError):
            mg.setupDDSerial(bad, mk(np.complex64, _pjs(mg, np.complex64, np.int64)))
    r = dsc.case(mg, "poisson2d_f32")
    rargs = (np.int64, r.mesh, r.boxes, r.overlap, mg.getNodalIndicesOfCell)
    for bad in (r.A.astype(np.float64), c.A):
        with pytest.raises(TypeError):
            mg.setupDDSerial(bad, mg.getDomainDecompositionParam(np.float32, *rargs, _pjs(mg, np.float32), singleValues=True))
    with pytest.raises(NotImplementedError):                             # the operator-constructor branch stays unmirrored
        mg.setupDDSerial(c.A.toarray(), mk(np.complex64, _pjs(mg, np.complex64)))


def test_solve_refuses_other_dtypes_before_the_device(mg):
    """b and x of exactly the param's dtype: everything else is a TypeError raised ahead of the upload (so also without a GPU)."""
    for name in ("helmholtz2d_c32_t0", "poisson2d_f32"):
        c = dsc.case(mg, name)
        p = c.dd_param(mg)
        n = c.A.shape[0]
        good = np.zeros(n, dtype=c.VAL)
        for bad in (np.zeros(n, dtype=c.wide), np.zeros(n, dtype=np.complex64 if c.VAL is np.float32 else np.float32), [0.0] * n):
            with pytest.raises(TypeError):
                mg.solveDDSerial(c.A, bad, good.copy(), p)
            with pytest.raises(TypeError):
                mg.solveDDSerial(c.A, good, bad, p)
        with pytest.raises(TypeError):                                   # the operator of the sweep must be the param's dtype too
            mg.solveDDSerial(c.A.astype(c.wide), good, good.copy(), p)
        assert p._handle is None


def test_mixed_closure_dtypes(mg, monkeypatch):
    """getDDpreconditioner (DomainDecomposition.jl:136-146): x0 and rt in VAL, x_new in eltype(B) - a complex128 B with a complex64
    param narrows r, sweeps in single from zero and widens the result.  (The sweep itself is replaced here: no device.)"""
    DD = mg.DomainDecomposition
    c = dsc.case(mg, "helmholtz2d_c32_t0")
    p = c.dd_param(mg)
    seen = []

    def fake(A, b, x, DDparam, niter=1, doTranspose=0):
        seen.append((b.dtype, x.dtype, float(np.abs(x).max()), niter, doTranspose, b.copy()))
        x[...] = 2 * b
        return x, DDparam

    monkeypatch.setattr(DD, "solveDDSerial", fake)
    B = (np.arange(c.A.shape[0]) * (1 + 1e-9) + 0.25j).astype(np.complex128)
    out = DD.getDDpreconditioner(c.A, p, B, 1)(B)
    assert out.dtype == np.complex128 and seen[0][:5] == (np.complex64, np.complex64, 0.0, 1, 1)
    assert np.array_equal(seen[0][5], B.astype(np.complex64)) and np.array_equal(out, (2 * B.astype(np.complex64)).astype(np.complex128))
    out32 = DD.getDDpreconditioner(c.A, p, B.astype(np.complex64))(B.astype(np.complex64))
    assert out32.dtype == np.complex64


def test_new_symbols_declared_exported_and_bound(mg, built):
    header = open(HEADER).read()
    lib = mg.device.load_library()
    for name, argtypes in NEW.items():
        assert re.search(rf"\bmg_status\s+{name}\s*\(", header), name   # declared
        assert hasattr(lib, name), name                                 # exported
        restype, args = mg.device.SIGNATURES[name]                      # bound with these argument types
        assert restype is C.c_int and list(args) == argtypes, name
    v, one = np.ones(2, dtype=np.float32), np.ones(2, dtype=np.int64)
    f32, i64, u32 = mg.device._f32, mg.device._i64, mg.device._u32
    for name in NEW:                                                     # a null handle / null out is refused before any device call
        if "create" in name:
            assert getattr(lib, name)(0, 1, i64(one), i64(one), f32(v), 1, i64(one), u32(np.ones(2, dtype=np.uint32)), i64(one), None) == 1
        elif "set_factor" in name:
            I = u32 if name.endswith("UINT32") else i64
            ix = np.ones(2, dtype=np.uint32 if name.endswith("UINT32") else np.int64)
            assert getattr(lib, name)(None, 1, 1, i64(one), I(ix), f32(v), i64(one), I(ix), f32(v), I(ix), I(ix)) == 1
        elif "dd0" in name:
            assert getattr(lib, name)(None, None, None, 1, 0) == 1
        else:
            assert getattr(lib, name)(None, None, None, 1, 1, 0) == 1


@pytest.mark.parametrize("name", list(dsc.CASES))
def test_fixture_guard(mg, name):
    """err(reference) <= REF_ERR_MAX on every case of the GPU file, after one sweep and after three: a condition on the inputs."""
    c = dsc.case(mg, name)
    E, X = c.E(), c.reference()
    for s in dsc.SWEEPS:
        e = dsc.err(X[s], E[s])
        print(f"{name} after {s} sweep(s): err(reference) {e:.2e}")
        assert X[s].dtype == np.dtype(c.VAL) and 0.0 < e <= dsc.REF_ERR_MAX


def test_stored_reference_iterates_are_the_binarys(mg):
    """The stored file holds one single vector per case and iterate - and, where the reference binary is built, what it returns."""
    Z = np.load(dsc.GOLDEN)
    assert sorted(Z.files) == sorted(f"{n}_s{s}" for n in dsc.CASES for s in dsc.SWEEPS)
    for n in dsc.CASES:
        c = dsc.case(mg, n)
        assert all(Z[f"{n}_s{s}"].dtype == np.dtype(c.VAL) and Z[f"{n}_s{s}"].shape == c.b.shape for s in dsc.SWEEPS)
    for name in ("poisson2d_f32", "helmholtz2d_c32_t1") if os.path.exists(dsc.REF_SO) else ():
        X = dsc.case(mg, name).reference_sweeps()
        for s in dsc.SWEEPS:
            assert np.array_equal(Z[f"{name}_s{s}"], X[s])


def _single_param(mg, LU):
    A, mesh = helmholtz(mg, [16, 16], 0.5, 0.5)
    p = mg.getMGparam(np.complex128, np.int64, 2, 8, 8, 1e-6, "Jac", 0.8, 2, 2, "V", "NoMUMPS", 0.5, 0.0, singlePrecision=True)
    p.LU = LU
    return A, mesh, p


def _dd_lu32(mg, mesh, boxes, overlap):
    return mg.getDomainDecompositionParam(np.complex64, np.int64, mesh, boxes, overlap, mg.getNodalIndicesOfCell,
                                          _pjs(mg, np.complex64, np.int64), singleValues=True)


def test_define_coarsest_ainv(mg):
    """A ComplexF32 DomainDecompositionParam preset as param.LU of a singlePrecision param is set up on the complex64 coarsest
    operator and stays the caller's object; a ComplexF64 one keeps today's NotImplementedError; a ComplexF32 one on a ComplexF64
    param is a TypeError."""
    DD = mg.DomainDecomposition
    A, mesh, p = _single_param(mg, None)
    LU = p.LU = _dd_lu32(mg, mesh, [2, 2], [1, 1])
    mg.MGsetup(A, mesh, p)
    try:
        Ac = p.As[-1]
        assert p.LU is LU and Ac.dtype == np.complex64 and not DD.isempty(LU) and len(LU.PrecParams) == 4
        assert list(LU.Mesh.n) == list(p.Meshes[-1].n)
        s = LU.PrecParams[0].Ainv
        I = LU.GlobalIndices[0].astype(np.int64) - 1
        F = dsc.single_layout(dsc.factor(sp.csr_matrix(Ac)[I][:, I].astype(np.complex128)), "CFP32_INT64")
        assert s.L.dtype == np.complex64 and np.array_equal(s.L.data, F["Lv"]) and np.array_equal(s.U.data, F["Uv"])
        q = mg.copySolver(p)                                             # the solver object is copied with its keyword, without its setup
        assert isinstance(q.LU, DD.DomainDecompositionParam) and q.LU is not LU and q.LU.singleValues and DD.isempty(q.LU)
        mg.destroyCoarsestLU(p)                                          # cleared and kept, as for ComplexF64
        assert p.LU is LU and DD.isempty(LU)
    finally:
        mg.clear_(p)
    A, mesh, p = _single_param(mg, None)
    p.LU = csc.dd_lu(mg, mesh, [2, 2], [1, 1], np.complex128)            # the default-path pin
    with pytest.raises(NotImplementedError):
        mg.MGsetup(A, mesh, p)
    pd = mg.getMGparam(np.complex128, np.int64, 2, 8, 8, 1e-6, "Jac", 0.8, 2, 2, "V", "NoMUMPS", 0.5, 0.0)
    pd.LU = _dd_lu32(mg, mesh, [2, 2], [1, 1])
    with pytest.raises(TypeError):
        mg.MGsetup(A, mesh, pd)


def test_default_paths_are_unchanged(mg):
    mesh = _mesh(mg)
    with pytest.raises(TypeError):
        mg.getDomainDecompositionParam(np.complex64, np.int64, mesh, [2, 2], [1, 1])
    A, _, b = dd_cases.poisson(mg, [8, 8])
    p = dd_cases.dd_param(mg, A, mesh, [2, 2], [1, 1])                   # a double param still takes what it took
    assert not p.is_single and p.PrecParams[0].Ainv.L.dtype == np.float64
    cx = mg.ParallelJuliaSolver.getParallelJuliaSolver(np.complex128, np.int64)
    with pytest.raises(NotImplementedError):
        mg.setupDDSerial(A, mg.getDomainDecompositionParam(np.float64, np.int64, mesh, [2, 2], [1, 1], mg.getNodalIndicesOfCell, cx))
