"""The Vanka cell-block smoother on the device (mg_vanka_*, csrc/mg_vanka.hpp) against the numpy restatement of the Julia
serial path (tests/vanka_cases.py) and, for the fixture's cases, against what the reference's compiled primitives gave
(vanka_outputs.npz).  Bound: relative max-norm 1e-12, the project's bound for a restatement (tests/test_dd_gpu.py).  Every
check is made after one iteration from a random x and again after two more from that iterate."""
import ctypes as C

import numpy as np
import pytest

import vanka_cases as V

pytestmark = pytest.mark.gpu

TOL = 1e-12
MG_ERR_INVALID, MG_ERR_UNSUPPORTED = 1, 4


def _err(a, ref):
    return np.abs(a - ref).max() / np.abs(ref).max()


def _check_sweeps(mg, A, D, n, ip, vtype, x0, b, numit=1, refs=None, what=""):
    """One call of `numit` iterations from x0, then a call of two more from that iterate, device vs restatement (and the stored
    reference x where given)."""
    xd = x0.copy()
    xr = x0.copy()
    for step, its in enumerate((numit, 2)):
        mg.RelaxVankaFacesColor(A, xd, b, D, its, 1, np.asarray(n), ip, vtype)
        V.restate_relax(A, xr, b, D, its, n, ip, vtype)
        e = _err(xd, xr)
        print(f"{what} n={n} ip={ip} type={vtype} call {step + 1} ({its} it): rel. max-norm error {e:.3e}")
        assert e <= TOL
        if refs is not None:
            er = _err(xd, refs[step])
            print(f"    against the reference primitives: {er:.3e}")
            assert er <= TOL
    return xd


SMALL = [([6, 4], False), ([6, 4], True), ([5, 7], False), ([5, 7], True),
         ([4, 3, 5], False), ([4, 3, 5], True), ([6, 5, 4], False), ([6, 5, 4], True)]
TYPES = [("rb_scalar", V.FULL_VANKA_RB, 0.6, 1), ("rb_tuple", V.FULL_VANKA_RB, (0.7, 0.5), 1), ("econ", V.ECON_VANKA_RB, 0.8, 1),
         ("add", V.FULL_VANKA_ADD, 0.6, 2)]          # ADD with numit = 2: the stale y shows


@pytest.mark.parametrize("n,ip", SMALL, ids=[f"{'x'.join(map(str, n))}{'m' if ip else 'f'}" for n, ip in SMALL])
@pytest.mark.parametrize("tname,vtype,w,numit", TYPES, ids=[t[0] for t in TYPES])
def test_small_meshes(mg, n, ip, tname, vtype, w, numit):
    A = V.mixed_operator(n, ip)
    D = mg.setupVankaFacesPreconditioner(A, np.asarray(n), w, ip, vtype)
    N = A.shape[0]
    _check_sweeps(mg, A, D, n, ip, vtype, V.seeded(N, 21), V.seeded(N, 22), numit, what=tname)


@pytest.mark.parametrize("n", [[64, 48], [24, 20, 16]], ids=["64x48", "24x20x16"])
@pytest.mark.parametrize("tname,vtype,w,numit", TYPES, ids=[t[0] for t in TYPES])
def test_several_workgroups(mg, n, tname, vtype, w, numit):
    """A colour spans several workgroups and a partial last one."""
    A = V.mixed_operator(n, True)
    D = mg.setupVankaFacesPreconditioner(A, np.asarray(n), w, True, vtype)
    N = A.shape[0]
    _check_sweeps(mg, A, D, n, True, vtype, V.seeded(N, 31), V.seeded(N, 32), numit, what=tname)


@pytest.mark.parametrize("name", list(V.REF_CASES))
def test_against_reference_primitives(mg, name):
    n, ip, cx, seed = V.REF_CASES[name]
    A, x0, b, D = V.ref_inputs(mg, name)
    G = np.load(V.GOLDEN)
    assert int(G[name + "_seed"]) == seed
    _check_sweeps(mg, A, D, n, ip, V.FULL_VANKA_RB, x0, b, 1, refs=(G[name + "_x1"], G[name + "_x3"]), what=name)


@pytest.mark.parametrize("n", [[6, 4], [4, 3, 5]], ids=["6x4", "4x3x5"])
@pytest.mark.parametrize("tname,vtype,w,numit", TYPES, ids=[t[0] for t in TYPES])
def test_complex(mg, n, tname, vtype, w, numit):
    A = V.mixed_operator(n, True, omega=V.REF_OMEGA)
    D = mg.setupVankaFacesPreconditioner(A, np.asarray(n), w, True, vtype)
    assert D.dtype == np.complex64
    N = A.shape[0]
    _check_sweeps(mg, A, D, n, True, vtype, V.seeded(N, 41, True), V.seeded(N, 42, True), numit, what=tname)


@pytest.mark.parametrize("vtype", [V.FULL_VANKA_RB, V.FULL_VANKA_ADD])
def test_numit_zero_and_identical_bits(mg, vtype):
    n = [24, 20, 16]
    A = V.mixed_operator(n, True)
    D = mg.setupVankaFacesPreconditioner(A, np.asarray(n), 0.6, True, vtype)
    N = A.shape[0]
    x0, b = V.seeded(N, 51), V.seeded(N, 52)
    x = x0.copy()
    mg.RelaxVankaFacesColor(A, x, b, D, 0, 1, np.asarray(n), True, vtype)
    assert np.array_equal(x, x0)                       # numit = 0 does nothing
    runs = []
    for _ in range(2):
        x = x0.copy()
        mg.RelaxVankaFacesColor(A, x, b, D, 2, 1, np.asarray(n), True, vtype)
        runs.append(x)
    assert np.array_equal(runs[0], runs[1]) and not np.array_equal(runs[0], x0)


def _create(mg, A, D, n, ip, nrows=None):
    lib = mg.device.load_library()
    cp = np.ascontiguousarray(A.indptr, dtype=np.int64) + 1
    rv = np.ascontiguousarray(A.indices, dtype=np.int64) + 1
    nz = np.ascontiguousarray(A.data, dtype=np.float64)
    blk = np.asfortranarray(D, dtype=np.float32)
    nn = np.ascontiguousarray(n, dtype=np.int64)
    h = C.c_void_p()
    rc = lib.mg_vanka_create_FP64_INT64(0, nn.size, nn.ctypes.data_as(C.POINTER(C.c_longlong)), 1 if ip else 0,
                                        A.shape[0] if nrows is None else nrows, cp.ctypes.data_as(C.POINTER(C.c_longlong)),
                                        rv.ctypes.data_as(C.POINTER(C.c_longlong)), nz.ctypes.data_as(C.POINTER(C.c_double)),
                                        blk.ctypes.data_as(C.POINTER(C.c_float)), C.byref(h))
    return lib, rc, h


@pytest.mark.parametrize("n,ip,bs,colours,live", [([6, 4], True, 5, 4, 4), ([5, 7], False, 4, 4, 4), ([4, 3, 5], True, 7, 8, 8),
                                                  ([6, 1, 4], False, 6, 8, 4)])
def test_info(mg, n, ip, bs, colours, live):
    A = V.mixed_operator(n, ip)
    D = mg.setupVankaFacesPreconditioner(A, np.asarray(n), 0.6, ip)
    lib, rc, h = _create(mg, A, D, n, ip)
    assert rc == 0
    try:
        info = mg.vanka.vanka_info(h)
        assert info[:7] == [0, bs, int(np.prod(n)), colours, 2 * live, 1, A.shape[0]] and info[7] == 0
        x, b = V.seeded(A.shape[0], 61), V.seeded(A.shape[0], 62)
        dp = C.POINTER(C.c_double)
        assert lib.mg_vanka_apply_FP64(h, x.ctypes.data_as(dp), b.ctypes.data_as(dp), 3, V.FULL_VANKA_RB) == 0
        assert mg.vanka.vanka_info(h)[7] == 3 * 2 * live
        assert lib.mg_vanka_apply_FP64(h, x.ctypes.data_as(dp), b.ctypes.data_as(dp), 3, V.FULL_VANKA_ADD) == 0
        assert mg.vanka.vanka_info(h)[7] == 3 * 2 * live + 1 + 3
    finally:
        lib.mg_vanka_destroy(h)


def test_bad_sizes_and_lex_launch_nothing(mg):
    n, ip = [6, 4], True
    A = V.mixed_operator(n, ip)
    D = mg.setupVankaFacesPreconditioner(A, np.asarray(n), 0.6, ip)
    for bad_n, bad_ip in (([6, 5], True), ([6, 4], False), ([6, 4, 1], True)):
        lib, rc, h = _create(mg, A, D, bad_n, bad_ip)
        assert rc == MG_ERR_INVALID and not h.value and lib.mg_last_error()
    lib, rc, h = _create(mg, A, D, n, ip)
    assert rc == 0
    try:
        x0, b = V.seeded(A.shape[0], 71), V.seeded(A.shape[0], 72)
        dp = C.POINTER(C.c_double)
        for vtype in (V.FULL_VANKA_LEX, 2, 17):
            x = x0.copy()
            assert lib.mg_vanka_apply_FP64(h, x.ctypes.data_as(dp), b.ctypes.data_as(dp), 1, vtype) == MG_ERR_UNSUPPORTED
            assert np.array_equal(x, x0) and mg.vanka.vanka_info(h)[7] == 0
        assert lib.mg_vanka_apply_FP64(h, x.ctypes.data_as(dp), x.ctypes.data_as(dp), 1, V.FULL_VANKA_RB) == MG_ERR_INVALID
        assert lib.mg_vanka_apply_CFP64(h, x.ctypes.data_as(dp), b.ctypes.data_as(dp), 1, V.FULL_VANKA_RB) == 3   # MG_ERR_STATE
        assert mg.vanka.vanka_info(h)[7] == 0
    finally:
        lib.mg_vanka_destroy(h)
