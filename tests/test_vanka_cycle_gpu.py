"""The Vanka smoother inside the cycle (relaxation type 2 of the device library): recursiveCycle and solveMG on hierarchies
built by MGsetup with the Systems transfer operators, against the numpy V-cycle of tests/vanka_cases.py that calls the
restatement of the Julia serial relaxation.  Bound: relative max-norm 1e-12, as in tests/test_vanka_gpu.py.

The contraction is a property of the input, checked on the restatement itself: with w = 0.6 (the reference's
testGMGforElasticityVanka.jl), lambda = mu = 1 and V(1,1) its residual falls by 0.14, 0.21, 0.21, 0.24, 0.29 per cycle on
32 x 32 (3 levels; W-cycle: 0.13 ... 0.24) and by 0.14, 0.23, 0.26, 0.29, 0.32 on 16 x 16 x 16 (2 levels)."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import vanka_cases as V

pytestmark = pytest.mark.gpu

TOL = 1e-12
CASES = {"2d_v": ([32, 32], 3, "V"), "3d_v": ([16, 16, 16], 2, "V"), "2d_w": ([32, 32], 3, "W")}
_cache = {}


def _setup(mg, name):
    """(param, b, restatement's first and second cycle, restatement's x and residual history of 5 cycles), computed once."""
    if name not in _cache:
        n, levels, cyc = CASES[name]
        A = V.mixed_operator(n, True)
        M = mg.getRegularMesh([0, 1] * len(n), n)
        p = mg.getMGparam(np.float64, np.int64, levels, 1, 5, 1e-30, "VankaFaces", 0.6, 1, 1, cyc, "NoMUMPS", 0.4, 0.0,
                          "SystemsFacesMixedLinear")
        mg.MGsetup(A, M, p)
        assert p.levels == levels
        b = V.seeded(A.shape[0], 5)
        ns = [list(map(int, m.n)) for m in p.Meshes]
        lu = spla.splu(sp.csc_matrix(p.As[-1]))
        c1 = V.restate_vcycle(p.As, p.Ps, p.Rs, p.relaxPrecs, ns, True, V.FULL_VANKA_RB, lu, b, None, True, 1, 1, cyc)
        c2 = V.restate_vcycle(p.As, p.Ps, p.Rs, p.relaxPrecs, ns, True, V.FULL_VANKA_RB, lu, b, c1.copy(), False, 1, 1, cyc)
        xs, res = V.restate_solve(p, b, 5, cyc)
        for a in (c1, c2, xs, res):
            a.setflags(write=False)
        _cache[name] = (p, b, c1, c2, xs, res)
    return _cache[name]


def _err(a, ref):
    return np.abs(a - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_contracts(mg, name):
    """The condition on the input (CPU arithmetic only): the restatement's own residual falls in each of the five cycles."""
    res = _setup(mg, name)[5]
    print(name, "factors", res[1:] / res[:-1])
    assert np.all(res[1:] < 0.5 * res[:-1])


@pytest.mark.parametrize("name", list(CASES))
def test_recursive_cycle(mg, name):
    p, b, c1, c2, _, _ = _setup(mg, name)
    x = np.zeros_like(b)
    mg.recursiveCycle(p, b, x)
    e1 = _err(x, c1)
    mg.recursiveCycle(p, b, x)
    e2 = _err(x, c2)
    print(f"{name}: first cycle {e1:.3e}, second cycle {e2:.3e}")
    assert e1 <= TOL and e2 <= TOL


@pytest.mark.parametrize("name", list(CASES))
def test_solve_mg_history(mg, name):
    p, b, _, _, xs, res = _setup(mg, name)
    x = np.zeros_like(b)
    _, _, iters = mg.solveMG(p, b, x)
    assert iters == 5
    e = np.abs(p.resvec - res).max() / res[0]
    ex = _err(x, xs)
    print(f"{name}: residual history {e:.3e}, x {ex:.3e}")
    assert p.resvec.shape == res.shape and np.all(np.abs(p.resvec - res) <= TOL * res[0]) and ex <= TOL


def test_preconditioner_and_krylov(mg):
    """getMultigridPreconditioner is one cycle from zero; the Krylov driver that accepts relax type 1 runs with type 2."""
    p, b, c1, _, _, _ = _setup(mg, "2d_v")
    Mfun = mg.getMultigridPreconditioner(p, b)
    assert _err(Mfun(b), c1) <= TOL
    x = np.zeros_like(b)
    old = p.relativeTol
    p.relativeTol = 1e-8
    try:
        _, _, it, resvec = mg.solveGMRES_MG(p.As[0], p, b, x, True, 5)
    finally:
        p.relativeTol = old
    assert np.linalg.norm(b - p.As[0] @ x) <= 1e-6 * np.linalg.norm(b)


def test_unserved_combinations_raise(mg):
    n = [32, 32]
    A = V.mixed_operator(n, True)
    M = mg.getRegularMesh([0, 1, 0, 1], n)
    b = V.seeded(A.shape[0], 5)
    p = mg.getMGparam(np.float64, np.int64, 3, 1, 5, 1e-8, "VankaFaces", 0.6, 1, 1, "K", "NoMUMPS", 0.4, 0.0, "SystemsFacesMixedLinear")
    mg.MGsetup(A, M, p)
    with pytest.raises(NotImplementedError):
        mg.solveMG(p, b, np.zeros_like(b))
    p = mg.getMGparam(np.float64, np.int64, 3, 1, 5, 1e-8, "VankaFaces", 0.6, 1, 1, "V", "NoMUMPS", 0.4, 0.0, "SystemsFacesMixedLinear")
    mg.MGsetup(A, M, p)
    B = np.asfortranarray(np.stack([b, b], axis=1))
    with pytest.raises(NotImplementedError):
        mg.solveMG(p, B, np.zeros_like(B, order="F"))
    # the library refuses them too: the K-cycle and a block of right-hand sides with relaxation type 2
    mg.adjustMemoryForNumRHS(p, 1)
    dev = mg.to_device(p)
    lib = dev.lib
    assert lib.mg_set_cycle_type(dev.handle, ord("K")) == 0 and lib.mg_finalize(dev.handle) == 0
    x = np.zeros_like(b)
    assert lib.mg_cycle_FP64(dev.handle, mg.device._f64(b), mg.device._f64(x), b.size, 1, 1) == 4     # MG_ERR_UNSUPPORTED
    assert lib.mg_set_cycle_type(dev.handle, ord("V")) == 0 and lib.mg_finalize(dev.handle) == 0
    assert lib.mg_set_nrhs(dev.handle, 2) == 0
    X = np.zeros_like(B, order="F")
    assert lib.mg_cycle_FP64(dev.handle, mg.device._f64(B), mg.device._f64(X), b.size, 2, 1) == 4     # MG_ERR_UNSUPPORTED
    assert not X.any() and lib.mg_set_nrhs(dev.handle, 1) == 0
    mg.recursiveCycle(p, b, x)                                                                        # the handle still serves
    assert np.linalg.norm(b - p.As[0] @ x) < np.linalg.norm(b)
