"""CPU: the ``blockKcycle`` switch, the declarations of mg_block_fgmres_relax_CF64 / _CF32, and the Kronecker oracle of
tests/complex_kcycle_block_cases.py - with the conditions on the inputs of tests/test_complex_kcycle_block_gpu.py asserted on the
oracle alone.

What is asserted about the inputs (never about a device):
  * the Kronecker param with k = 1 gives the vector oracle's bits (the construction changes nothing by itself);
  * at block scale 1.0 and at BREAK_SCALE = 1e-11 no residual estimate of the two cycles lies within a factor 4 of the break's 1e-5
    (complex_kcycle_oracle.rn_clear_of_tol), and at 1e-11 every relaxation breaks after its first direction;
  * the columns of a block are coupled: the block result differs from the column-by-column result by more than 1e-4 of max|X| -
    so an implementation that serves a block column by column cannot pass the GPU tests' 1e-11."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import complex_kcycle_block_cases as KB
import complex_kcycle_oracle as korc
from complex_cases import complex_rhs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(prob, s) for prob in ("3lev", "4lev") for s in KB.SCHEDULES]


def test_flag(mg):
    base = (np.complex128, np.int64, 3, 8, 5, 1e-6, "Jac-GMRES", 0.8, 2, 1, "K")
    assert mg.getMGparam(*base).blockKcycle is False
    p = mg.getMGparam(*base, blockKcycle=True)
    assert p.blockKcycle is True and p.VAL == np.complex128
    q = mg.copySolver(p)
    assert q.blockKcycle is True and q.cycleType == "K" and q.relaxType == "Jac-GMRES"
    assert mg.copySolver(mg.getMGparam(*base)).blockKcycle is False
    s = mg.getMGparam(*base, singlePrecision=True, singleKcycle=True, blockKcycle=True)
    assert s.blockKcycle is True and s.VAL == np.complex64 and mg.copySolver(s).blockKcycle is True
    with pytest.raises(NotImplementedError, match="blockKcycle"):
        mg.getMGparam(np.float64, np.int64, 3, 8, 5, 1e-6, "Jac", 0.8, 2, 1, "K", blockKcycle=True)      # a real VAL
    with pytest.raises(TypeError):
        mg.getMGparam(*base, "NoMUMPS", 0.4, 0.0, "FullWeighting", True)       # keyword only


def test_entry_points_are_exported_declared_and_bound(mg, built):
    lib = mg.device.load_library()
    header = open(os.path.join(ROOT, "include", "mgvcycle.h")).read()
    dp, ll = C.POINTER(C.c_double), C.c_longlong
    args = [C.c_void_p, ll, dp, dp, ll, ll, ll, C.c_double, dp, dp, dp, C.POINTER(ll), dp, dp]
    for name in ("mg_block_fgmres_relax_CF64", "mg_block_fgmres_relax_CF32"):
        fn = getattr(lib, name)                                   # exported
        assert re.search(rf"\bmg_status\s+{name}\s*\(", header)   # declared
        restype, argtypes = mg.device.SIGNATURES[name]            # bound
        assert restype is C.c_int and list(argtypes) == args
        assert fn.restype is C.c_int and list(fn.argtypes) == args
        assert fn(None, 1, None, None, 1, 1, 1, 1e-5, None, None, None, None, None, None) != 0 and lib.mg_last_error()   # null handle
    assert "kcycle_blocks" in header


def test_device_guard_honours_the_flag(mg):
    """ComplexDeviceHierarchy._block_guard on bare objects (no device is touched): refused without the flag, served with it, and
    Vanka with 'K' refused either way."""
    cls = mg.device.ComplexDeviceHierarchy
    for sched in (("K", "Jac"), ("V", "Jac-GMRES"), ("K", "Jac-GMRES")):
        d = cls.__new__(cls)
        d._schedule = sched
        with pytest.raises(NotImplementedError, match="K-cycle / Jac-GMRES"):
            d._block_guard()
        with pytest.raises(NotImplementedError, match="K-cycle / Jac-GMRES"):
            d.block_fgmres_relax(1, np.zeros((4, 2), dtype=np.complex128), np.zeros((4, 2), dtype=np.complex128), 2)
        d._kcycle_blocks = True
        d._block_guard()
        d._vanka = d._vanka_blocks = True
        with pytest.raises(NotImplementedError, match="K-cycle / Jac-GMRES"):
            d._block_guard()
    d = cls.__new__(cls)
    d._schedule = ("V", "Jac")
    d._block_guard()


def test_kron_param_with_one_column_is_the_vector_oracle(mg):
    for prob, sched in (("3lev", ("Jac-GMRES", "K", 2, 1)), ("4lev", ("SPAI", "K", 2, 1))):
        p = KB.cycle_param(mg, prob, sched)
        b = complex_rhs(p.As[0].shape[0], 9)
        tv, tk = [], []
        xv = korc.recursiveCycle(p, b, np.zeros_like(b), 1, trace=tv).copy()
        xk = korc.recursiveCycle(KB.kron_param(p, 1), b, np.zeros_like(b), 1, trace=tk).copy()
        assert xv.tobytes() == xk.tobytes() and tv == tk and len(tv) > 0


@pytest.mark.parametrize("k", KB.KS)
@pytest.mark.parametrize("prob,sched", CASES, ids=KB.case_id)
def test_clearances_of_the_cycle_cases(mg, prob, sched, k):
    ref = KB.two_cycles(mg, prob, sched, k, 1.0)
    assert len(ref["trace"]) > 0 and korc.rn_clear_of_tol(ref["trace"], 4.0), korc.all_rn(ref["trace"])
    assert korc.all_rn(ref["trace"]).min() >= 4 * korc.GMRES_TOL          # no break at this scale
    brk = KB.two_cycles(mg, prob, sched, k, KB.BREAK_SCALE)
    assert len(brk["trace"]) > 0 and korc.rn_clear_of_tol(brk["trace"], 4.0), korc.all_rn(brk["trace"])
    assert all(rec[3] == 1 for rec in brk["trace"]) and korc.all_rn(brk["trace"]).max() <= korc.GMRES_TOL / 4
    print(f"{prob} {sched} k={k}: clearance {korc.all_rn(ref['trace']).min() / korc.GMRES_TOL:.0f} at scale 1, "
          f"{korc.GMRES_TOL / korc.all_rn(brk['trace']).max():.0f} at scale {KB.BREAK_SCALE}")


@pytest.mark.parametrize("prob,sched", [("3lev", ("Jac-GMRES", "V", 2, 2)), ("4lev", ("Jac-GMRES", "K", 2, 1)), ("4lev", ("Jac", "K", 2, 1))],
                         ids=KB.case_id)
def test_the_columns_of_a_block_are_coupled(mg, prob, sched):
    ref = KB.two_cycles(mg, prob, sched, 3, 1.0)
    Xc = KB.columnwise_cycle(ref["p"], ref["B"])
    scale = np.abs(ref["X1"]).max()
    diff = np.abs(ref["X1"] - Xc).max() / scale
    col1 = np.abs(ref["X1"][:, 1] - Xc[:, 1]).max() / np.abs(Xc[:, 1]).max()
    print(f"{prob} {sched}: block against column-wise {diff:.2e} of max|X|, column 1 {col1:.2e} relative")
    assert diff > 1e-4


def test_relaxation_inputs(mg):
    """The relaxation cases of the GPU test: cond(H) <= 1e8 on numpy's H, no break at scale 1, a break after one direction at 1e-9."""
    for name in ("awkward5000", "oneblock100"):
        p = KB.relax_param(mg, name)
        A, d = p.As[0], p.relaxPrecs[0]
        for k in (1, 3, 4, 16):
            R0, X0 = KB.relax_block(A.shape[0], k)
            _, _, H, _ = KB.relax_bases(A, d, R0, 8)
            assert np.linalg.cond(H) <= 1e8
            _, rn = KB.relax_oracle(A, d, R0, X0, 8)
            assert len(rn) == 8 and min(rn) > 4e-5
    p = KB.relax_param(mg, "awkward5000")
    A, d = p.As[0], p.relaxPrecs[0]
    R0, _ = KB.relax_block(A.shape[0], 3, scale=1e-9)
    _, rn = KB.relax_oracle(A, d, R0, np.zeros_like(R0), 3)
    assert len(rn) == 1 and rn[0] < 1e-5 / 4
