"""ComplexF64 factor applier (mg_lu_*_CFP64 <-> applyLUsolve_CFP64_INT64, deps/src/parLU.cpp:69-72,193-260) without a GPU:
the C ABI's surface, the mirror's type rules, and the pin of the reference binary - binary against stored outputs against
scipy, plain and adjoint, one and several right-hand sides."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from parlu_complex_cases import GOLDEN, REF_SO, factor, pinned_cases, ref_lu_solve_complex_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgvcycle.h")
NEW = ["mg_lu_create_CFP64_INT64", "mg_lu_solve_CFP64", "mg_lu_solve_dev_CFP64"]
CF64 = {"mg_create_CF64", "mg_set_operator_CF64_INT64", "mg_set_relax_CF64", "mg_set_coarse_dense_inverse_CF64",
        "mg_set_coarse_lu_CF64_INT64", "mg_cycle_CF64", "mg_solve_CF64", "mg_spmv_CF64"}


def test_cfp64_lu_symbols_exported_declared_and_bound(mg, built):
    header = open(HEADER).read()
    declared = set(re.findall(r"\bint\s+(mg_\w+)\s*\(", header))
    lib = mg.device.load_library()
    for n in NEW + ["mg_lu_form", "mg_lu_time_dev", "mg_lu_destroy"]:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in mg.device.SIGNATURES, n
    assert set(re.findall(r"\bint\s+(mg_\w+_CF64\w*)\s*\(", header)) == CF64     # the hierarchy's complex surface is unchanged


def test_c_abi_refuses_bad_arguments_before_touching_a_device(mg, built):
    import ctypes as C
    lib = mg.device.load_library()
    h = C.c_void_p()
    one = np.ones(2, dtype=np.int64)
    v = np.ones(2)
    I, F = mg.device._i64, mg.device._f64
    assert lib.mg_lu_create_CFP64_INT64(0, 1, I(one), I(one), F(v), I(one), I(one), F(v), I(one), I(one), None) == 1
    assert lib.mg_lu_create_CFP64_INT64(0, 0, I(one), I(one), F(v), I(one), I(one), F(v), I(one), I(one), C.byref(h)) == 1
    assert lib.mg_lu_create_CFP64_INT64(0, 1, None, I(one), F(v), I(one), I(one), F(v), I(one), I(one), C.byref(h)) == 1
    zero = np.zeros(2, dtype=np.int64)                                            # 0-based row pointers
    assert lib.mg_lu_create_CFP64_INT64(0, 1, I(zero), I(one), F(v), I(zero), I(one), F(v), I(one), I(one), C.byref(h)) == 1
    assert b"1-based" in lib.mg_last_error()
    assert lib.mg_lu_solve_CFP64(None, F(v), F(v), 1, 1, 0) == 1
    assert lib.mg_lu_solve_dev_CFP64(None, None, None, 1, 1, 0) == 1
    assert not h.value


def test_mirror_types_without_a_device(mg, built):
    PJ = mg.ParallelJuliaSolver
    LU = PJ.getParallelJuliaSolver(np.complex128, np.int64, numCores=2, backend=3)
    assert np.dtype(LU.VAL) == np.complex128 and LU.backend == 3 and LU.nFac == 0
    for VAL in (np.complex64, np.float32):
        with pytest.raises(TypeError):
            PJ.getParallelJuliaSolver(VAL, np.int64)
    with pytest.raises(TypeError):
        PJ.getParallelJuliaSolver(np.complex128, np.uint32)
    z = np.zeros(3, dtype=np.complex128)
    with pytest.raises(RuntimeError):
        PJ.solve(z, z.copy(), LU)                                  # not factored
    with pytest.raises(TypeError):
        PJ.solve(np.zeros(3), z.copy(), LU)                        # real b into a complex solver
    with pytest.raises(TypeError):
        PJ.solve(z, np.zeros(3), LU)                               # real x
    with pytest.raises(TypeError):
        PJ.solve(z.astype(np.complex64), z.copy(), LU)
    with pytest.raises(TypeError):
        PJ.solveLinearSystem(sp.identity(3, format="csc"), np.zeros(3), LU)
    LR = PJ.getParallelJuliaSolver()
    with pytest.raises(TypeError):
        PJ.solve(z, np.zeros(3), LR)                               # complex b into a real solver
    with pytest.raises(TypeError):
        PJ.solve(np.zeros(3), z.copy(), LR)
    with pytest.raises(TypeError):
        PJ.setupLUFactor(sp.identity(3, format="csc") * (1.0 + 1.0j), LR)
    c = PJ.copySolver(LU)
    assert np.dtype(c.VAL) == np.complex128 and c.L is None
    assert PJ.clear_(LU).L is None


@pytest.mark.parametrize("case", pinned_cases(), ids=lambda c: c[0])
def test_reference_binary_stored_outputs_and_scipy_agree(case):
    """The reference's compiled applyLUsolve_CFP64_INT64 against its stored outputs (not stale where the binary is built)
    against scipy: doTranspose = 1 is the ADJOINT solve (A^H x = b), not the plain transpose."""
    name, A, B, t = case
    lu = factor(A)
    stored = np.load(GOLDEN)[name]
    if os.path.exists(REF_SO):
        X = ref_lu_solve_complex_block(lu, B, t)
        assert X.shape == stored.shape
        assert np.abs(X - stored).max() <= 1e-12 * np.abs(X).max(), "stored output is stale: rerun make_parlu_complex_outputs.py"
    else:
        X = stored
    ref = lu.solve(B, trans="H" if t else "N")
    assert np.abs(X - ref).max() <= 1e-12 * np.abs(ref).max()
    Aop = A.conj().T if t else A
    assert np.abs(Aop @ X - B).max() <= 1e-10 * np.abs(B).max()
    if t and name.startswith("helmholtz"):                          # the operator tells the adjoint from the transpose
        assert np.abs(A.T @ X - B).max() > 1e-3 * np.abs(B).max()
