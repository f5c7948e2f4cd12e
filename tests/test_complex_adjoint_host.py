"""adjointHierarchy of complex hierarchies, host side (no GPU): the host mirror of MGsetup.jl:274-318 for complex VAL (``'`` is the
adjoint) on ComplexF64 and singlePrecision params, its routing to a resident hierarchy - checked with a stub in ``param.device`` that
records its calls -, the two entry points mg_adjoint_hierarchy_CF64 / _CF32 as the header declares them, and the route
``solveLinearSystem_`` takes for a complex MGsolver with sym != 1.

The operator: helmholtz([16, 12, 10], k h = 0.5, damping 0.5) plus the one-sided super-diagonal perturbation of
tests/test_transpose_device.py, times 1 + 0.3i: complex, non-symmetric and non-Hermitian, three levels."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import complex_oracle as corc
from complex_adjoint_cases import adjoint_sorted, base_operator, base_param, oracle_param, same_csr
from complex_cases import complex_rhs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgvcycle.h")
MG_ERR_INVALID = 1

CASES = [(relax, coarse, single) for relax in ("Jac", "SPAI") for coarse in ("NoMUMPS", "GMRES") for single in (False, True)]


@pytest.mark.parametrize("relax,coarse,single", CASES)
def test_adjoint_hierarchy_host_mirror(mg, relax, coarse, single):
    """Fails without the feature: AttributeError."""
    p, A, _ = base_param(mg, relax, coarse, single)
    cdt, rdt = (np.complex64, np.float32) if single else (np.complex128, np.float64)
    As0 = [M.copy() for M in p.As]
    Ps0 = [M.copy() for M in p.Ps]
    Rs0 = [M.copy() for M in p.Rs]
    d0 = [np.array(d, copy=True) for d in p.relaxPrecs]
    LU0 = np.array(p.LU, copy=True) if coarse == "GMRES" else None
    assert p.doTranspose == 0
    mg.adjointHierarchy(p)
    assert p.doTranspose == 1
    for l in range(3):
        assert p.As[l].dtype == cdt and same_csr(p.As[l], adjoint_sorted(As0[l]))
        assert p.As[l].has_sorted_indices
    for l in range(2):
        assert p.relaxPrecs[l].dtype == cdt and np.array_equal(p.relaxPrecs[l], np.conj(d0[l]))
        assert p.Ps[l].dtype == rdt and p.Rs[l].dtype == rdt
        assert np.array_equal(p.Ps[l].toarray(), Rs0[l].toarray().T)
        assert same_csr(p.Rs[l], Rs0[l])                                   # the reference's literal pair of assignments
    nc = p.As[-1].shape[0]
    if coarse == "GMRES":
        assert p.LU.dtype == LU0.dtype and np.array_equal(p.LU, np.conj(LU0))
    else:
        bc = complex_rhs(nc, 3)
        z = p.LU.solve(bc)
        Act = As0[-1].astype(np.complex128).conj().T
        assert np.linalg.norm(Act @ z - bc) <= 1e-12 * np.linalg.norm(bc)
    # convergence on A' x = b: the oracle's solveMG on the flipped param
    b = complex_rhs(A.shape[0], 9)
    x = np.zeros_like(b)
    hist = {}
    q = oracle_param(p)
    corc.solveMG(q, b, x, hist)
    rv = hist["resvec"]
    A0 = As0[0].astype(np.complex128)                                      # (the operator the hierarchy holds: rounded for single)
    true = np.linalg.norm(A0.conj().T @ x - b)
    print(f"  {relax} {coarse} single={single}: resvec[-1] / resvec[0] = {rv[-1] / rv[0]:.2e} after {len(rv) - 1} cycles")
    # Ps[l] = Rs[l]' is 2^-dim times the prolongation the setup built (the reference's literal assignments), so the coarse correction
    # of the flipped hierarchy is damped eightfold: as a stand-alone iteration it brings the residual of A' x = b down to about 0.09
    # of its start within five cycles and stays there (with Ps rescaled by 2^dim it contracts like the forward cycle, 6e-5 in 12
    # cycles: measured with this oracle).  No rate is claimed; what is asserted is that the residual it reduces is that of A'.
    assert rv[-1] < rv[1] < rv[0]
    assert abs(true - rv[-1]) <= 1e-8 * rv[0]
    # the second flip: As back bit for bit, doTranspose 0, Ps[l] = Rs[l]' again
    mg.adjointHierarchy(p)
    assert p.doTranspose == 0
    for l in range(3):
        assert same_csr(p.As[l], As0[l])
    for l in range(2):
        assert np.array_equal(p.relaxPrecs[l], d0[l])
        assert np.array_equal(p.Ps[l].toarray(), Rs0[l].toarray().T) and same_csr(p.Rs[l], Rs0[l])
    if coarse == "GMRES":
        assert np.array_equal(p.LU, LU0)
    else:
        bc = complex_rhs(nc, 4)
        assert np.linalg.norm(As0[-1].astype(np.complex128) @ p.LU.solve(bc) - bc) <= 1e-12 * np.linalg.norm(bc)


def test_refusals(mg):
    A, mesh = mg.poisson_shifted([8, 8, 8])
    pr = mg.getMGparam(np.float64, np.int64, 3, 8, 6, 1e-10, "Jac", 0.8, 2, 1)
    mg.MGsetup(A, mesh, pr)
    with pytest.raises(TypeError, match="transposeHierarchy"):
        mg.adjointHierarchy(pr)
    p, _, _ = base_param(mg, "Jac", cells=(8, 8, 8))
    A0 = p.As[0].copy()
    p.relaxType = "Kaczmarz"
    with pytest.raises(RuntimeError, match="Not supported"):
        mg.adjointHierarchy(p)
    p.relaxType = "VankaFaces"
    with pytest.raises(NotImplementedError):
        mg.adjointHierarchy(p)
    p.relaxType = "Jac"
    assert p.doTranspose == 0 and same_csr(p.As[0], A0)                    # a refusal changes nothing


@pytest.mark.parametrize("single", [False, True])
def test_transpose_hierarchy_keeps_refusing_complex_params(mg, single):
    p, _, _ = base_param(mg, "Jac", single=single, cells=(8, 8, 8))
    with pytest.raises(NotImplementedError):
        mg.transposeHierarchy(p)
    assert mg.device.ComplexDeviceHierarchy.transpose_hierarchy is mg.device.ComplexDeviceHierarchy._refuse
    assert mg.device.ComplexDeviceHierarchy.adjoint_hierarchy is not mg.device.ComplexDeviceHierarchy._refuse
    assert mg.device.ComplexSingleDeviceHierarchy.adjoint_hierarchy is mg.device.ComplexDeviceHierarchy.adjoint_hierarchy


class StubDevice:
    """Stands in for a resident ComplexDeviceHierarchy."""

    def __init__(self, mg, fail=False):
        self.mg, self.fail = mg, fail
        self.calls, self.closed = [], 0

    def adjoint_hierarchy(self, param):
        self.calls.append((param.doTranspose, [M.copy() for M in param.As]))
        if self.fail:
            raise self.mg.device.MGDeviceError("stub: the device refuses")

    def close(self):
        self.closed += 1


def test_resident_hierarchy_is_flipped_and_kept(mg):
    """Fails without the feature (AttributeError); this is the routing a GPU-less machine can check."""
    p, _, _ = base_param(mg, "SPAI", cells=(8, 8, 8))
    A0 = p.As[0].copy()
    stub = p.device = StubDevice(mg)
    mg.adjointHierarchy(p)
    assert len(stub.calls) == 1 and stub.closed == 0 and p.device is stub
    flag, As_seen = stub.calls[0]
    assert flag == 1 and same_csr(As_seen[0], adjoint_sorted(A0))          # the device is called with the host mirror already flipped
    p.device = None


def test_device_error_releases_the_resident_hierarchy(mg):
    p, _, _ = base_param(mg, "SPAI", cells=(8, 8, 8))
    A0 = p.As[0].copy()
    stub = p.device = StubDevice(mg, fail=True)
    mg.adjointHierarchy(p)
    assert len(stub.calls) == 1 and stub.closed == 1 and p.device is None  # re-uploaded lazily by the next cycle
    assert p.doTranspose == 1 and same_csr(p.As[0], adjoint_sorted(A0))


def test_symbols_exported_and_declared(mg, built):
    names = ["mg_adjoint_hierarchy_CF64", "mg_adjoint_hierarchy_CF32"]
    header = open(HEADER).read()
    for n in names:
        assert re.search(r"\bmg_status\s+" + n + r"\s*\(\s*mg_hierarchy\s*\*\s*h\s*\)\s*;", header), n
        assert n in mg.device.SIGNATURES
    lib = mg.device.load_library()
    for n in names:
        assert hasattr(lib, n), n
    # the prototypes spelled `int` stay the eight of tests/test_complex_host.py
    eight = {"mg_create_CF64", "mg_set_operator_CF64_INT64", "mg_set_relax_CF64", "mg_set_coarse_dense_inverse_CF64",
             "mg_set_coarse_lu_CF64_INT64", "mg_cycle_CF64", "mg_solve_CF64", "mg_spmv_CF64"}
    assert set(re.findall(r"\bint\s+(mg_\w+_CF64\w*)\s*\(", header)) == eight
    assert "adjointHierarchy" in mg.__all__


def test_null_handle_is_invalid(mg, built):
    lib = mg.device.load_library()
    for fn in (lib.mg_adjoint_hierarchy_CF64, lib.mg_adjoint_hierarchy_CF32):
        assert fn(None) == MG_ERR_INVALID
        assert lib.mg_last_error()


def test_solve_linear_system_route(mg, monkeypatch):
    """A complex MGsolver with sym = 0: the first call with doTranspose = 1 sets up the ADJOINT conj(A)^T (not A^T), and a following
    call with doTranspose = 0 flips the hierarchy with adjointHierarchy, once."""
    from multigrid_jl_amd import wrappers
    A, mesh = base_operator(mg, (8, 8, 8))
    p = mg.getMGparam(np.complex128, np.int64, 3, 8, 6, 1e-8, "SPAI", 0.8, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
    s = mg.getMGsolver(p, mesh, 0, "BiCGSTAB")
    driven, flips = [], []

    def driver(As0, param, B, X, verbose=False):
        driven.append(As0.copy())
        return X, 0, 1, None

    real_adjoint = wrappers.adjointHierarchy
    monkeypatch.setattr(wrappers, "solveBiCGSTAB_MG_CFP64", driver)
    monkeypatch.setattr(wrappers, "adjointHierarchy", lambda param, *a: (flips.append(param.doTranspose), real_adjoint(param, *a))[1])
    monkeypatch.setattr(wrappers, "transposeHierarchy", lambda *a: pytest.fail("transposeHierarchy called for a complex solver"))
    b = complex_rhs(A.shape[0], 5)
    x = np.zeros_like(b)
    mg.solveLinearSystem_(A, b, x, s, 1)
    assert flips == [] and p.doTranspose == 1
    assert same_csr(p.As[0], adjoint_sorted(A)) and same_csr(driven[0], adjoint_sorted(A))
    mg.solveLinearSystem_(A, b, x, s, 0)
    assert flips == [1] and p.doTranspose == 0
    assert same_csr(p.As[0], A) and same_csr(driven[1], A)
    mg.solveLinearSystem_(A, b, x, s, 0)
    assert flips == [1] and len(driven) == 3                               # the same direction again: nothing flipped
    mg.solveLinearSystem_(A, b, x, s, 1)
    assert flips == [1, 0] and p.doTranspose == 1 and same_csr(driven[3], adjoint_sorted(A))
