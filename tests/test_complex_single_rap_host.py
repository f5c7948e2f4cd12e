"""The device re-setup of ComplexF32 hierarchies, host side (no GPU): the five _CF32 entry points and their argument types, the flag
``singleDeviceSetup`` in getMGparam / copySolver, the routing of ``replaceMatrixInHierarchy`` for a single param (a stub in
``param.device`` records the calls), and the refusals of a default single param, which stay what they were."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import complex_single_rap_cases as SR
from complex_cases import helmholtz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MG_ERR_INVALID = 1
FP, DP, LP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_longlong)


def test_the_five_entry_points_and_their_types(mg, built):
    """Fails without the feature: the parent's library exports none of them."""
    lib = mg.device.load_library()
    want = {"mg_rap_CF32": [C.c_void_p, FP, C.c_longlong, C.c_longlong, DP, LP],
            "mg_rap_level_ms_CF32": [C.c_void_p, DP, C.c_longlong],
            "mg_get_values_CF32": [C.c_void_p, C.c_longlong, C.c_longlong, FP, C.c_longlong],
            "mg_get_relax_CF32": [C.c_void_p, C.c_longlong, FP, C.c_longlong],
            "mg_replace_values_CF32": [C.c_void_p, C.c_longlong, C.c_longlong, FP, C.c_longlong]}
    header = open(os.path.join(ROOT, "include", "mgvcycle.h")).read()
    for name, argtypes in want.items():
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
        assert re.search(r"mg_status\s+%s\(mg_hierarchy\* h," % name, header), name
    f, d = np.zeros(4, dtype=np.float32), np.zeros(4)
    fp, dp = f.ctypes.data_as(FP), d.ctypes.data_as(DP)
    done = C.c_longlong(0)
    for call in (lambda: lib.mg_rap_CF32(None, fp, 2, 0, dp, C.byref(done)), lambda: lib.mg_rap_level_ms_CF32(None, dp, 1),
                 lambda: lib.mg_get_values_CF32(None, 1, 0, fp, 2), lambda: lib.mg_get_relax_CF32(None, 1, fp, 2),
                 lambda: lib.mg_replace_values_CF32(None, 1, 0, fp, 2)):
        assert call() == MG_ERR_INVALID
        assert lib.mg_last_error()


def test_flag_in_getMGparam_and_copySolver(mg):
    """Fails without the feature: the keyword is a TypeError there."""
    p = SR.single_param(mg, 3)
    assert p.singleDeviceSetup is True and p.singlePrecision and p.VAL == np.complex64
    assert SR.single_param(mg, 3, flag=False).singleDeviceSetup is False
    assert mg.getMGparam(np.complex128, np.int64, 3).singleDeviceSetup is False
    for VAL in (np.float64, np.complex128):
        with pytest.raises(NotImplementedError):
            mg.getMGparam(VAL, np.int64, 3, singleDeviceSetup=True)
    with pytest.raises(TypeError):                                   # keyword only
        mg.getMGparam(np.complex128, np.int64, 3, 8, 20, 1e-6, "SPAI", 1.0, 2, 2, "V", "NoMUMPS", 0.4, 0.0, "FullWeighting", True)
    q = mg.copySolver(p)
    assert q.singleDeviceSetup is True and q.singlePrecision
    assert mg.copySolver(SR.single_param(mg, 3, flag=False)).singleDeviceSetup is False
    g = SR.single_param(mg, 3, "Jac", 0.8, coarse="GMRES", coarseDeviceInverse=False)
    assert g.singleDeviceSetup and g.coarseSolveType == "GMRES"


class StubDevice:
    """Stands in for a resident ComplexSingleDeviceHierarchy: records the calls, refuses or does nothing."""

    def __init__(self, mg, fail=False):
        self.mg, self.fail, self.calls, self.closed = mg, fail, [], 0

    def replace_matrix(self, param, A_new):
        self.calls.append(A_new)
        if self.fail:
            raise self.mg.device.MGDeviceError("stub: the device refuses")
        param.As[0] = A_new

    def close(self):
        self.closed += 1


def _setup(mg, flag, relax="SPAI"):
    A, mesh = helmholtz(mg, [8, 8, 8], 0.5, 0.5)
    p = SR.single_param(mg, 3, relax, 0.8, flag=flag)
    mg.MGsetup(A, mesh, p)
    return p, A


def _same_bytes(p, q):
    assert len(p.As) == len(q.As) == 3
    for M, N in zip(p.As, q.As):
        assert M.dtype == N.dtype == np.complex64
        assert np.array_equal(M.indptr, N.indptr) and np.array_equal(M.indices, N.indices) and M.data.tobytes() == N.data.tobytes()
    for d, e in zip(p.relaxPrecs, q.relaxPrecs):
        assert d.dtype == e.dtype == np.complex64 and d.tobytes() == e.tobytes()
    for name in ("perm_r", "perm_c"):
        assert np.array_equal(getattr(p.LU, name), getattr(q.LU, name))
    for F in ("L", "U"):
        Lp, Lq = getattr(p.LU, F), getattr(q.LU, F)
        assert np.array_equal(Lp.indptr, Lq.indptr) and np.array_equal(Lp.indices, Lq.indices) and Lp.data.tobytes() == Lq.data.tobytes()


@pytest.mark.parametrize("relax", ["SPAI", "Jac"])
def test_flag_without_a_resident_device_is_the_host_path(mg, relax):
    p, A = _setup(mg, True, relax)
    q, _ = _setup(mg, False, relax)
    _same_bytes(p, q)                                                # (the setup does not look at the flag either)
    A2 = SR.new_matrix(A, 3)
    mg.replaceMatrixInHierarchy(p, A2)
    mg.replaceMatrixInHierarchy(q, A2)
    assert p.device is None and q.device is None
    _same_bytes(p, q)
    assert p.As[0].data.tobytes() == A2.data.tobytes()


def test_routing_of_a_resident_single_param(mg):
    A2 = None
    # with the flag: the device is asked, and kept
    p, A = _setup(mg, True)
    A2 = SR.new_matrix(A, 3)
    stub = p.device = StubDevice(mg)
    mg.replaceMatrixInHierarchy(p, A2)
    assert len(stub.calls) == 1 and stub.calls[0].dtype == np.complex64 and stub.closed == 0 and p.device is stub
    # without it: the host path, the device copy dropped - as before
    q, _ = _setup(mg, False)
    stub = q.device = StubDevice(mg)
    mg.replaceMatrixInHierarchy(q, A2)
    assert stub.calls == [] and stub.closed == 1 and q.device is None
    # the device refuses: the host path, with the bytes of a param that never had a device
    p, _ = _setup(mg, True)
    stub = p.device = StubDevice(mg, fail=True)
    mg.replaceMatrixInHierarchy(p, A2)
    assert len(stub.calls) == 1 and stub.closed == 1 and p.device is None
    _same_bytes(p, q)
    # another pattern: the host path
    import scipy.sparse as sp
    p, _ = _setup(mg, True)
    stub = p.device = StubDevice(mg)
    A3 = (A2.astype(np.complex128) + sp.csr_matrix(([0.25 + 0.5j], ([0], [A.shape[0] - 1])), shape=A.shape)).tocsr()
    A3.sort_indices()
    assert A3.nnz == A2.nnz + 1
    mg.replaceMatrixInHierarchy(p, A3)
    assert stub.calls == [] and stub.closed == 1 and p.device is None and p.As[0].dtype == np.complex64


def test_default_single_hierarchy_keeps_refusing(mg):
    """The four methods of ComplexSingleDeviceHierarchy without a device: an instance that never uploaded carries no flag and raises
    as before; one whose param carried the flag reaches the ComplexF64 methods' code (here: their first use of the missing handle)."""
    D = mg.device
    dev = D.ComplexSingleDeviceHierarchy.__new__(D.ComplexSingleDeviceHierarchy)
    assert dev._single_device_setup is False
    for call in (lambda: dev.replace_matrix(None, None), lambda: dev.replace_values(1, 0, None), lambda: dev.get_values(1, 0),
                 lambda: dev.rap_level_ms()):
        with pytest.raises(NotImplementedError):
            call()
    dev._single_device_setup = True
    dev._op_nnz = {}
    with pytest.raises(D.MGDeviceError):                             # (the served method: no such operator on this empty instance)
        dev.get_values(1, 0)
    for n in ("replace_matrix", "replace_values", "get_values", "rap_level_ms"):
        assert getattr(D.ComplexSingleDeviceHierarchy, n) is not getattr(D.ComplexDeviceHierarchy, n)
