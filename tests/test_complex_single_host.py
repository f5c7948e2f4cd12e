"""ComplexF32 hierarchies, host side (no GPU): the keyword and the types of the setup, the single-precision restatement
(tests/complex_single_oracle.py) pinned against the double cycle on the same rounded hierarchy, the numerical premise of the mixed
branch - a ComplexF64 Krylov method preconditioned by the single cycle keeps its iteration counts and its double accuracy - and
the exported _CF32 symbols."""
import os
import re

import numpy as np
import pytest

import complex_krylov_oracle as ck
import complex_oracle as corc
import complex_single_oracle as cs
from complex_cases import complex_rhs, helmholtz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgvcycle.h")


def _single_param(mg, levels=3, relax="SPAI", cyc="V"):
    return mg.getMGparam(np.complex128, np.int64, levels, 8, 6, 1e-6, relax, 0.8, 2, 1, cyc, "NoMUMPS", 0.5, 0.0, singlePrecision=True)


def test_keyword_flag_and_copy(mg):
    p = _single_param(mg)
    assert np.dtype(p.VAL) == np.complex64 and p.singlePrecision is True
    assert mg.mgdef.is_complex(p) and mg.mgdef.is_single(p)
    q = mg.copySolver(p)
    assert np.dtype(q.VAL) == np.complex64 and q.singlePrecision is True and q.cycleType == p.cycleType
    d = mg.getMGparam(np.complex128)
    assert np.dtype(d.VAL) == np.complex128 and d.singlePrecision is False and mg.mgdef.is_complex(d) and not mg.mgdef.is_single(d)
    assert mg.copySolver(d).singlePrecision is False
    with pytest.raises(TypeError, match="singlePrecision"):
        mg.getMGparam(np.complex64)
    with pytest.raises(NotImplementedError):
        mg.getMGparam(np.float64, singlePrecision=True)
    with pytest.raises(TypeError):
        mg.getMGparam(np.complex128, np.int64, 3, 8, 20, 1e-6, "SPAI", 1.0, 2, 2, "V", "NoMUMPS", 0.4, 0.0, "FullWeighting", True)


@pytest.mark.parametrize("relax", ["Jac", "SPAI"])
def test_setup_types(mg, relax):
    A, mesh = helmholtz(mg, [8] * 3, 0.5, 0.5)
    p = _single_param(mg, 3, relax)
    mg.MGsetup(A, mesh, p)

    def check():
        assert len(p.As) == 3
        assert all(M.dtype == np.complex64 for M in p.As)
        assert all(M.dtype == np.float32 for M in p.Ps + p.Rs)
        assert all(d.dtype == np.complex64 for d in p.relaxPrecs)
        nc = p.As[-1].shape[0]
        bc = complex_rhs(nc, 3)
        z = p.LU.solve(bc)
        assert z.dtype == np.complex128                         # factorised and solved in double
        Ac = p.As[-1].astype(np.complex128)
        assert np.linalg.norm(Ac @ z - bc) <= 1e-12 * np.linalg.norm(bc)

    check()
    # relaxPrecs come from the CONVERTED operator: the double formula on the single values, converted once
    ref = mg.getRelaxPrec(p.As[0].astype(np.complex128), relax, 0.8).astype(np.complex64)
    assert np.array_equal(p.relaxPrecs[0], ref)
    # every Galerkin product is the single product of the single operands
    Ac = (p.Rs[0] @ (p.As[0] @ p.Ps[0])).tocsr()
    Ac.sort_indices()
    assert Ac.dtype == np.complex64 and np.array_equal(Ac.data, p.As[1].data)
    A2, _ = helmholtz(mg, [8] * 3, 0.5, 0.3)
    mg.replaceMatrixInHierarchy(p, A2)
    check()
    assert np.array_equal(p.As[0].data, mg.mgsetup._as_csr(A2).astype(np.complex64).data)
    with pytest.raises(NotImplementedError):
        mg.transposeHierarchy(p)


@pytest.mark.parametrize("name", ["C1", "C3"])
def test_restatement_against_double_cycle_on_rounded_hierarchy(mg, name):
    """One single cycle from zero against the complex128 cycle on rounded(param) with b rounded to single: 64 * 2^-24 guards the
    restatement against an O(1) mistake (found when this was written: 1.0e-7 on C1, 6.4e-8 on C3)."""
    p, _, b = cs.case(mg, name)
    b32 = b.astype(np.complex64)
    x = cs.recursiveCycle(p, b32, np.zeros_like(b32), 1)
    assert x.dtype == np.complex64
    xo = corc.recursiveCycle(cs.rounded(p), b32.astype(np.complex128), np.zeros_like(b), 1)
    e = cs.rel2(x, xo)
    print(f"  {name}: single restatement vs double cycle on the rounded hierarchy: {e:.2e} (bound {64 * cs.U32:.2e})")
    assert e < 64 * cs.U32


def _premise(mg, name, method, inner=None):
    p, As, b = cs.case(mg, name)
    x, flag, count, rv = cs.reference(mg, name, method, inner)
    res = np.linalg.norm(b - As @ x) / np.linalg.norm(b)
    want = ck.EXPECTED[name]["bicgstab"][0] if method == "bicgstab" else ck.EXPECTED[name][inner]
    print(f"  {name} {method}{'' if inner is None else '(%d)' % inner}: {count} with the single M ({want} with the double M), "
          f"flag {flag}, true residual {res:.2e}")
    assert flag in (0, -3)
    assert res < 1e-8
    return count, want


@pytest.mark.parametrize("name", ["C1", "C2", "C3"])
def test_bicgstab_premise(mg, name):
    count, want = _premise(mg, name, "bicgstab")
    assert abs(count - want) <= 2


@pytest.mark.parametrize("name,inner", [("C1", 5), ("C1", 10), ("C2", 10), ("C3", 5), ("C3", 10)])
def test_fgmres_premise(mg, name, inner):
    count, want = _premise(mg, name, "fgmres", inner)
    assert abs(count - want) <= 1


def test_cf32_symbols_exported_and_declared(mg, built):
    names = ["mg_create_CF32", "mg_set_operator_CF32_INT64", "mg_set_relax_CF32", "mg_cycle_CF32", "mg_solve_CF32", "mg_spmv_CF32"]
    header = open(HEADER).read()
    declared = set(re.findall(r"\bint\s+(mg_\w+_CF32\w*)\s*\(", header))
    assert declared == set(names)
    lib = mg.device.load_library()
    for n in names:
        assert hasattr(lib, n), n
        assert n in mg.device.SIGNATURES
