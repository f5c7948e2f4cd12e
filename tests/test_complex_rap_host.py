"""replaceMatrixInHierarchy of ComplexF64 hierarchies, host side (no GPU): what the five entry points of the device path answer to a
null handle, and which path ``mgsetup.replaceMatrixInHierarchy`` takes for a complex param - checked with a stub in ``param.device``
that records its calls.  Every routing case ends with ``param.As`` / ``param.relaxPrecs`` equal to ``galerkin`` / ``getRelaxPrec`` on the
new matrix."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from complex_cases import helmholtz

MG_ERR_INVALID = 1


class StubDevice:
    """Stands in for a resident ComplexDeviceHierarchy: ``replace_matrix`` does on the host what the device does in HBM."""

    def __init__(self, mg, fail=False):
        self.mg, self.fail = mg, fail
        self.calls, self.closed = [], 0

    def replace_matrix(self, param, A_new):
        from multigrid_jl_amd.mgsetup import galerkin, _relax_param_arr
        self.calls.append(A_new)
        if self.fail:
            raise self.mg.device.MGDeviceError("stub: the device refuses")
        param.As[0] = A_new
        for l in range(len(param.As) - 1):
            param.relaxPrecs[l] = self.mg.getRelaxPrec(param.As[l], param.relaxType, _relax_param_arr(param)[l])
            param.As[l + 1] = galerkin(param.Rs[l], param.As[l], param.Ps[l])

    def close(self):
        self.closed += 1


def _setup(mg, VAL=np.complex128, relax="SPAI"):
    A, mesh = helmholtz(mg, [8, 8, 8], 0.5, 0.5)
    if VAL == np.float64:
        A = A.real.tocsr()
    p = mg.getMGparam(VAL, np.int64, 3, 8, 4, 1e-8, relax, 0.8, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(A, mesh, p)
    return p, A, mesh


def _new_values(A, seed=3):
    """Same pattern, non-symmetric new values of A's dtype."""
    rng = np.random.default_rng(seed)
    A2 = A.copy()
    f = 1.0 + 0.3 * rng.random(A.nnz)
    A2.data = A.data * (f + 0.2j * rng.random(A.nnz) if np.iscomplexobj(A.data) else f)
    return A2


def _assert_hierarchy_of(mg, p, A2):
    from multigrid_jl_amd.mgsetup import galerkin
    Al = A2
    assert np.array_equal(p.As[0].indices, A2.indices) and np.array_equal(p.As[0].data, A2.data)
    for l in range(len(p.As) - 1):
        assert np.array_equal(p.relaxPrecs[l], mg.getRelaxPrec(Al, p.relaxType, 0.8))
        Al = galerkin(p.Rs[l], Al, p.Ps[l])
        assert np.array_equal(Al.indices, p.As[l + 1].indices) and np.array_equal(Al.data, p.As[l + 1].data)
    x = np.arange(1.0, Al.shape[0] + 1).astype(Al.dtype)
    assert np.abs(Al @ p.LU.solve(x) - x).max() <= 1e-10 * np.abs(x).max()        # the coarsest factors are the new matrix's


def test_null_handle_is_invalid_for_the_five_entry_points(mg, built):
    """Fails without the feature: the parent's library exports none of them."""
    lib = mg.device.load_library()
    z = np.zeros(4)
    dp = z.ctypes.data_as(C.POINTER(C.c_double))
    done = C.c_longlong(0)
    calls = [lambda: lib.mg_rap_CF64(None, dp, 2, 0, dp, C.byref(done)),
             lambda: lib.mg_get_values_CF64(None, 1, 0, dp, 2),
             lambda: lib.mg_get_relax_CF64(None, 1, dp, 2),
             lambda: lib.mg_replace_values_CF64(None, 1, 0, dp, 2),
             lambda: lib.mg_replace_krylov_values_CFP64(None, dp, 2)]
    for call in calls:
        assert call() == MG_ERR_INVALID
        assert lib.mg_last_error()
    for n in ("replace_matrix", "replace_values", "get_values", "update_krylov_operator"):
        assert getattr(mg.device.ComplexDeviceHierarchy, n) is not mg.device.ComplexDeviceHierarchy._refuse, n
    assert mg.device.ComplexDeviceHierarchy.transpose_hierarchy is mg.device.ComplexDeviceHierarchy._refuse


def test_same_pattern_goes_to_the_device_and_keeps_it(mg):
    """Fails without the feature: the parent never calls the stub and releases it."""
    from multigrid_jl_amd.mgsetup import coarse_lu
    p, A, _ = _setup(mg)
    stub = p.device = StubDevice(mg)
    A2 = _new_values(A)
    mg.replaceMatrixInHierarchy(p, A2)
    assert len(stub.calls) == 1 and stub.closed == 0
    assert p.device is stub
    p.LU = coarse_lu(p.As[-1])                                            # (the stub factors nothing)
    _assert_hierarchy_of(mg, p, A2)


def test_other_pattern_takes_the_host_path(mg):
    p, A, _ = _setup(mg)
    stub = p.device = StubDevice(mg)
    A2 = _new_values(A)
    A2 = (A2 + sp.csr_matrix(([0.25 + 0.5j], ([0], [A.shape[0] - 1])), shape=A.shape)).tocsr()
    A2.sort_indices()
    assert A2.nnz == A.nnz + 1
    mg.replaceMatrixInHierarchy(p, A2)
    assert stub.calls == [] and stub.closed == 1 and p.device is None
    _assert_hierarchy_of(mg, p, A2)


def test_device_error_falls_back_to_the_host_path(mg):
    p, A, _ = _setup(mg)
    stub = p.device = StubDevice(mg, fail=True)
    A2 = _new_values(A)
    mg.replaceMatrixInHierarchy(p, A2)
    assert len(stub.calls) == 1 and stub.closed == 1 and p.device is None
    _assert_hierarchy_of(mg, p, A2)


def test_schwarz_coarsest_solver_stays_on_the_host_path(mg):
    from multigrid_jl_amd.domain_decomposition import DomainDecompositionParam
    from multigrid_jl_amd import mgsetup
    p, A, _ = _setup(mg)
    stub = p.device = StubDevice(mg)
    dd = DomainDecompositionParam.__new__(DomainDecompositionParam)       # (only its type is looked at before the coarsest setup)
    p.LU = dd
    seen = []
    orig = mgsetup.defineCoarsestAinv
    mgsetup.defineCoarsestAinv = lambda param, Ac: seen.append(Ac)        # the Schwarz setup itself is not what is tested here
    try:
        A2 = _new_values(A)
        mg.replaceMatrixInHierarchy(p, A2)
    finally:
        mgsetup.defineCoarsestAinv = orig
    assert stub.calls == [] and stub.closed == 1 and p.device is None
    assert len(seen) == 1 and seen[0] is p.As[-1]
    p.LU = mgsetup.coarse_lu(p.As[-1])
    _assert_hierarchy_of(mg, p, A2)


def test_float64_param_is_unaffected(mg):
    from multigrid_jl_amd.mgsetup import coarse_lu
    p, A, _ = _setup(mg, np.float64)
    stub = p.device = StubDevice(mg)
    A2 = _new_values(A)
    mg.replaceMatrixInHierarchy(p, A2)
    assert len(stub.calls) == 1 and stub.closed == 0 and p.device is stub     # the FP64 device path, as before
    p.LU = coarse_lu(p.As[-1])
    _assert_hierarchy_of(mg, p, A2)
    p.device = None
