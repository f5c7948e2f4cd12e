"""Single-precision factor applier (mg_lu_*_FP32 / _CFP32 <-> applyLUsolve_FP32_UINT32, _CFP32_UINT32, _CFP32_INT64,
deps/src/parLU.cpp:33-46, 85-115) without a GPU: the C ABI's surface, the mirror's type rules with and without
``singleFactors``, the layout setupLUFactor leaves, and the pin of the reference binary - binary against stored outputs
against the substitution in double (parlu_single_cases)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from parlu_complex_cases import REF_SO, helmholtz_unsymmetric, nonsymmetric50
from parlu_single_cases import (FORMS, GOLDEN, REF_ERR_MAX, case, create_args, err, pinned_cases, ref_lu_solve_single,
                                single_layout)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgvcycle.h")
NEW = ["mg_lu_create_FP32_UINT32", "mg_lu_create_CFP32_UINT32", "mg_lu_create_CFP32_INT64", "mg_lu_solve_FP32",
       "mg_lu_solve_dev_FP32", "mg_lu_solve_CFP32", "mg_lu_solve_dev_CFP32", "mg_set_coarse_lu_CF32_INT64"]
MG_ERR_INVALID = 1


def test_single_lu_symbols_exported_declared_and_bound(mg, built):
    declared = set(re.findall(r"\b(?:int|mg_status)\s+(mg_\w+)\s*\(", open(HEADER).read()))
    lib = mg.device.load_library()
    for n in NEW:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in mg.device.SIGNATURES, n


@pytest.mark.parametrize("form", list(FORMS))
def test_c_abi_refuses_bad_arguments_before_touching_a_device(mg, built, form):
    lib = mg.device.load_library()
    create = getattr(lib, "mg_lu_create_" + form)
    IND = FORMS[form][1]
    h = C.c_void_p()
    ptr1, ptr0 = np.ones(2, dtype=np.int64), np.zeros(2, dtype=np.int64)
    F = dict(Lp=ptr1, Lc=np.ones(2, dtype=IND), Lv=np.ones(4, dtype=np.float32), Up=ptr1, Uc=np.ones(2, dtype=IND),
             Uv=np.ones(4, dtype=np.float32), p=np.ones(2, dtype=IND), q=np.ones(2, dtype=IND))
    args = create_args(mg, F, form)
    assert create(0, 1, *args, None) == MG_ERR_INVALID                                  # out is null
    assert create(0, 0, *args, C.byref(h)) == MG_ERR_INVALID                            # empty factor
    for k in range(len(args)):                                                          # any null array
        assert create(0, 1, *args[:k], None, *args[k + 1:], C.byref(h)) == MG_ERR_INVALID
    assert create(0, 1, *create_args(mg, dict(F, Lp=ptr0, Up=ptr0), form), C.byref(h)) == MG_ERR_INVALID
    assert b"1-based" in lib.mg_last_error()
    assert not h.value
    v = np.ones(2, dtype=np.float32)
    f32 = mg.device._f32
    for name in ("mg_lu_solve_FP32", "mg_lu_solve_CFP32"):
        assert getattr(lib, name)(None, f32(v), f32(v), 1, 1, 0) == MG_ERR_INVALID
    for name in ("mg_lu_solve_dev_FP32", "mg_lu_solve_dev_CFP32"):
        assert getattr(lib, name)(None, None, None, 1, 1, 0) == MG_ERR_INVALID
    one = np.ones(2, dtype=np.int64)
    i64 = mg.device._i64
    assert lib.mg_set_coarse_lu_CF32_INT64(None, 1, i64(one), i64(one), f32(v), i64(one), i64(one), f32(v), i64(one),
                                           i64(one)) == MG_ERR_INVALID


@pytest.mark.parametrize("form", list(FORMS))
def test_order_mismatch_is_refused_before_a_device_is_needed(mg, built, form):
    """Row pointers that do not end on a 1-based count for the order n given (n = 1 with pointers written for n = 0, a
    pointer array that runs backwards) are MG_ERR_INVALID before a device is looked for."""
    lib = mg.device.load_library()
    create = getattr(lib, "mg_lu_create_" + form)
    IND = FORMS[form][1]
    h = C.c_void_p()
    good = np.array([1, 2], dtype=np.int64)
    one_i, one_v = np.ones(2, dtype=IND), np.ones(4, dtype=np.float32)
    for bad in (np.array([1, 0], dtype=np.int64), np.array([1, -3], dtype=np.int64)):
        for F in (dict(Lp=bad, Up=good), dict(Lp=good, Up=bad)):
            F.update(Lc=one_i, Lv=one_v, Uc=one_i, Uv=one_v, p=one_i, q=one_i)
            assert create(0, 1, *create_args(mg, F, form), C.byref(h)) == MG_ERR_INVALID
            assert not h.value


def test_mirror_types_with_and_without_single_factors(mg, built):
    PJ = mg.ParallelJuliaSolver
    for VAL, IND in ((np.float32, np.uint32), (np.complex64, np.uint32), (np.complex64, np.int64), (np.float32, np.int64)):
        with pytest.raises(TypeError):
            PJ.getParallelJuliaSolver(VAL, IND)                       # refused without the keyword, as before
    for VAL, IND in ((np.float32, np.int64), (np.complex128, np.uint32), (np.float64, np.uint32)):
        with pytest.raises(TypeError):
            PJ.getParallelJuliaSolver(VAL, IND, singleFactors=True)   # the reference has no such form
    assert PJ.getParallelJuliaSolver(np.float64, np.int64, singleFactors=True).singleFactors is False   # nothing single asked for
    for form, (VAL, IND, _) in FORMS.items():
        LU = PJ.getParallelJuliaSolver(VAL, IND, numCores=2, backend=3, singleFactors=True)
        assert np.dtype(LU.VAL) == VAL and np.dtype(LU.IND) == IND and LU.singleFactors and LU.backend == 3
        z = np.zeros(3, dtype=VAL)
        with pytest.raises(RuntimeError):
            PJ.solve(z, z.copy(), LU)                                 # not factored
        wide = np.complex128 if VAL is np.complex64 else np.float64
        other = np.float32 if VAL is np.complex64 else np.complex64
        for bad in (wide, other, np.int64):                           # nothing is cast
            with pytest.raises(TypeError):
                PJ.solve(z.astype(bad), z.copy(), LU)
            with pytest.raises(TypeError):
                PJ.solve(z, z.astype(bad), LU)
            with pytest.raises(TypeError):
                PJ.solveLinearSystem(sp.identity(3, format="csc"), z.astype(bad), LU)
        c = PJ.copySolver(LU)
        assert c.singleFactors and np.dtype(c.VAL) == VAL and np.dtype(c.IND) == IND and c.L is None
        assert PJ.clear_(LU).L is None
    with pytest.raises(TypeError):
        PJ.setupLUFactor(sp.identity(3, format="csc") * (1.0 + 1.0j),
                         PJ.getParallelJuliaSolver(np.float32, np.uint32, singleFactors=True), upload=False)


@pytest.mark.parametrize("form", list(FORMS))
def test_setup_lu_factor_layout(mg, built, form):
    """setupLUFactor(upload=False): L, U of VAL, p, q of IND, L's diagonal last and U's first, A[p, q] = L U to single
    rounding (the factorisation itself is double); copySolver carries factors and flag.  A real matrix goes through the
    complex forms converted."""
    PJ = mg.ParallelJuliaSolver
    VAL, IND, _ = FORMS[form]
    for A in (nonsymmetric50(), helmholtz_unsymmetric()):
        if A.dtype.kind == "c" and VAL is np.float32:
            A = sp.csc_matrix(A.real)
        LU = PJ.setupLUFactor(A, PJ.getParallelJuliaSolver(VAL, IND, singleFactors=True), upload=False)
        assert LU.L.dtype == VAL and LU.U.dtype == VAL and LU.p.dtype == IND and LU.q.dtype == IND and LU._handle is None
        n = A.shape[0]
        assert sorted(LU.p.tolist()) == list(range(1, n + 1)) and sorted(LU.q.tolist()) == list(range(1, n + 1))
        assert all(LU.L.indices[LU.L.indptr[r + 1] - 1] == r and LU.U.indices[LU.U.indptr[r]] == r for r in range(n))
        p, q = LU.p.astype(np.int64) - 1, LU.q.astype(np.int64) - 1
        Apq = sp.csr_matrix(A)[p][:, q].toarray()
        LUd = (LU.L.astype(np.complex128) @ LU.U.astype(np.complex128)).toarray()
        # every entry of L U is a sum of products of single-rounded values: 2^-23 relative per product, summed over a row of
        # |L| |U| (bounded by its largest entry times the longest row)
        bound = 2.0 ** -23 * (abs(LU.L).astype(np.float64) @ abs(LU.U).astype(np.float64)).toarray().max()
        assert np.abs(Apq - LUd).max() <= bound
        c = PJ.copySolver(LU)
        assert c.singleFactors and c.L.dtype == VAL and c.p.dtype == IND and (c.L != LU.L).nnz == 0 and c.L is not LU.L


@pytest.mark.parametrize("key", pinned_cases(), ids=lambda k: f"{k[0]}-nrhs{k[1]}-t{k[2]}")
def test_reference_binary_stored_outputs_and_double_substitution_agree(key):
    """The reference's compiled single entry points against their stored outputs (equal where the binary is built) against
    the substitution in double: err(reference) <= 1e-5, the condition guarding the fixture."""
    form, nrhs, t = key
    name, F, B, E = case(form, nrhs, t)
    stored = np.load(GOLDEN)[name]
    assert stored.dtype == FORMS[form][0] and stored.shape == B.shape
    if os.path.exists(REF_SO):
        X = ref_lu_solve_single(F, B, form, t)
        assert np.array_equal(X, stored), "stored output is stale: rerun make_parlu_single_outputs.py"
    else:
        X = stored
    e = err(X, E)
    print(f"{name}: err(reference) {e:.3e}")
    assert e <= REF_ERR_MAX


@pytest.mark.parametrize("t", [0, 1])
@pytest.mark.parametrize("nrhs", [1, 5])
def test_reference_uint32_and_int64_entries_give_equal_bits(nrhs, t):
    """applyLUsolve_CFP32_UINT32 and applyLUsolve_CFP32_INT64 on equal inputs: equal bits (the stored outputs where the binary
    is not built)."""
    _, Fi, B, _ = case("CFP32_INT64", nrhs, t)
    _, Fu, Bu, _ = case("CFP32_UINT32", nrhs, t)
    assert np.array_equal(B, Bu) and np.array_equal(Fi["Lv"], Fu["Lv"]) and np.array_equal(Fi["Lc"], Fu["Lc"])
    if os.path.exists(REF_SO):
        Xi, Xu = ref_lu_solve_single(Fi, B, "CFP32_INT64", t), ref_lu_solve_single(Fu, B, "CFP32_UINT32", t)
    else:
        z = np.load(GOLDEN)
        Xi, Xu = z[case("CFP32_INT64", nrhs, t)[0]], z[case("CFP32_UINT32", nrhs, t)[0]]
    assert np.array_equal(Xi, Xu)


def test_single_layout_rounds_once(mg):
    """The helper's factors are the double factors rounded to single - the conversion of parallelJuliaSolver.jl:137-145 - and
    the mirror's setupLUFactor gives the same arrays."""
    PJ = mg.ParallelJuliaSolver
    A = helmholtz_unsymmetric()
    from parlu_complex_cases import factor
    F = single_layout(factor(A), "CFP32_UINT32")
    LU = PJ.setupLUFactor(A, PJ.getParallelJuliaSolver(np.complex64, np.uint32, singleFactors=True), upload=False)
    assert np.array_equal(F["Lv"], LU.L.data) and np.array_equal(F["Uv"], LU.U.data)
    assert np.array_equal(F["Lc"], LU.L.indices + 1) and np.array_equal(F["p"], LU.p) and np.array_equal(F["q"], LU.q)
