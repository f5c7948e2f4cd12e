"""-m "not gpu": the device build of the coarsest operator's inverse, as far as it goes without a device - the declared and exported
symbols, the new keyword of getMGparam, the argument checks that precede the first device call, and the conditions the inputs of
the GPU tests (tests/coarse_inverse_cases.py) are meant to meet."""
import ctypes as C
import os

import numpy as np
import pytest

import coarse_inverse_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mg_dense_inverse_FP64", "mg_dense_inverse_CF64", "mg_build_coarse_dense_inverse_FP64",
               "mg_build_coarse_dense_inverse_CF64", "mg_get_coarse_dense_inverse_FP64", "mg_get_coarse_dense_inverse_CF64"]
MG_ERR_INVALID, MG_ERR_STATE, MG_ERR_UNSUPPORTED = 1, 3, 4
_dp = C.POINTER(C.c_double)


def test_symbols_declared_and_exported(mg, built):
    header = open(os.path.join(ROOT, "include", "mgvcycle.h")).read()
    lib = mg.device.load_library()
    for name in NEW_SYMBOLS:
        assert f"mg_status {name}(" in header
        assert getattr(lib, name).restype is C.c_int
    for key in ("coarse_device_inverse", "coarse_device_inverse_max"):
        assert key in open(os.path.join(ROOT, "multigrid.jl_amd", "csrc", "mg_types.inc")).read()
    assert callable(mg.device.dense_inverse)
    assert hasattr(mg.device.DeviceHierarchy, "coarse_dense_inverse") and hasattr(mg.device.ComplexDeviceHierarchy, "coarse_dense_inverse")


@pytest.mark.parametrize("val,single", [(np.float64, False), (np.complex128, False), (np.complex128, True)], ids=["FP64", "CF64", "CF32"])
def test_keyword_of_getMGparam(mg, val, single):
    kw = {"singlePrecision": True} if single else {}
    args = (val, np.int64, 3, 1, 5, 1e-8, "Jac", 0.8, 2, 1, "V")
    p = mg.getMGparam(*args, **kw)
    assert p.coarseDeviceInverse is False and mg.copySolver(p).coarseDeviceInverse is False
    q = mg.getMGparam(*args, coarseDeviceInverse=True, **kw)
    assert q.coarseDeviceInverse is True and mg.copySolver(q).coarseDeviceInverse is True
    assert mg.copySolver(q).singlePrecision == single
    with pytest.raises(TypeError):                       # keyword only
        mg.getMGparam(*args, "NoMUMPS", 0.4, 0.0, "FullWeighting", True)
    with pytest.raises(NotImplementedError):
        mg.getMGparam(*args, "GMRES", coarseDeviceInverse=True, **kw)


def test_argument_checks_without_a_device(mg, built):
    lib = mg.device.load_library()
    a = np.eye(2, order="F")
    z = np.zeros((2, 2), order="F")
    for fn in (lib.mg_dense_inverse_FP64, lib.mg_dense_inverse_CF64):
        assert fn(0, 2, None, z.ctypes.data_as(_dp)) == MG_ERR_INVALID
        assert fn(0, 2, a.ctypes.data_as(_dp), None) == MG_ERR_INVALID
        assert fn(0, 0, a.ctypes.data_as(_dp), z.ctypes.data_as(_dp)) == MG_ERR_INVALID
        assert fn(0, -3, a.ctypes.data_as(_dp), z.ctypes.data_as(_dp)) == MG_ERR_INVALID
        assert fn(0, 8193, a.ctypes.data_as(_dp), z.ctypes.data_as(_dp)) == MG_ERR_UNSUPPORTED
        assert b"8192" in lib.mg_last_error()
    for fn in (lib.mg_build_coarse_dense_inverse_FP64, lib.mg_build_coarse_dense_inverse_CF64):
        assert fn(None) == MG_ERR_INVALID
    for fn in (lib.mg_get_coarse_dense_inverse_FP64, lib.mg_get_coarse_dense_inverse_CF64):
        assert fn(None, 2, z.ctypes.data_as(_dp)) == MG_ERR_INVALID
    assert np.array_equal(z, np.zeros((2, 2)))           # nothing was written
    with pytest.raises(ValueError):
        mg.device.dense_inverse(np.zeros((2, 3)))


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
def test_conditions_of_the_gpu_inputs(cx):
    """Every matrix handed to a GPU test: cond_2 <= 1e4 and numpy inverts it; the exact case's inverse is exact."""
    for n in K.SIZES:
        A = K.matrix(n, cx)
        assert A.shape == (n, n) and (n == 1 or np.all(A.diagonal() == 0))
        cond = np.linalg.cond(A)
        r = K.res(A, np.linalg.inv(A))
        print(f"n={n} cx={cx}: cond_2 {cond:.2e}, numpy residual {r:.2e}, floor {n * K.EPS:.2e}")
        assert cond <= K.COND_MAX and r <= 1e-10
    for n in (5, 70, 130):
        A, X = K.exact_case(n, cx)
        assert np.array_equal(A @ X, np.eye(n)) and np.array_equal(X @ A, np.eye(n))
        assert np.count_nonzero(A) == n and (not cx or np.count_nonzero(A.real == 0) > n * n - n)
    Z, N = K.singular_cases(cx)
    assert np.linalg.matrix_rank(Z) == 69 and np.isnan(N).sum() == 1


def test_coarsest_operators_of_the_hierarchies(mg):
    """The coarsest operators the GPU tests invert: their orders, cond_2 <= 1e4."""
    want = {"8x8": 25, "8x8x8": 125, "16x16x16": 729, "real8x8x8": 125}
    for name in K.HCASES:
        A, mesh = K.operator(mg, name)
        p = K.param(mg, name)
        mg.MGsetup(A, mesh, p)
        Ac = p.As[-1].toarray()
        cond = np.linalg.cond(Ac)
        print(f"{name}: coarsest order {Ac.shape[0]}, cond_2 {cond:.2e}, numpy residual {K.res(Ac, np.linalg.inv(Ac)):.2e}")
        assert p.levels == 2 and Ac.shape[0] == want[name] and cond <= K.COND_MAX
        assert p.device is None                           # (the set-up alone touches no device)
