"""Pins the numpy restatement of the Julia serial relaxation (tests/vanka_cases.py) to the reference's compiled primitives:
vanka_outputs.npz holds what getVankaVariablesOfCell, cs2loc, computeResidualAtIdx_* and updateSolution_* of deps/src/Vanka.c
gave when driven through the serial schedule of Vanka.jl:406-424 (tests/golden/reference_binaries/make_vanka_outputs.py).
Only the .npz is read.  Bound: relative max-norm 1e-12, the project's bound for a restatement (tests/test_dd_gpu.py); the
restatement sits at 1e-16 .. 6e-16 of the stored x on these cases."""
import numpy as np
import pytest

import vanka_cases as V

TOL = 1e-12


@pytest.fixture(scope="module")
def golden():
    return np.load(V.GOLDEN)


def test_fixture_holds_every_case(golden):
    for name, (n, ip, cx, seed) in V.REF_CASES.items():
        assert int(golden[name + "_seed"]) == seed
        assert golden[name + "_x1"].dtype == (np.complex128 if cx else np.float64)
    assert {(tuple(n), ip, cx) for n, ip, cx, _ in V.REF_CASES.values()} >= {((6, 4), True, False), ((5, 7), False, False),
                                                                            ((4, 3, 5), True, False), ((6, 4), True, True),
                                                                            ((5, 7), False, True), ((4, 3, 5), True, True)}


@pytest.mark.parametrize("name", list(V.REF_CASES))
def test_index_lists_equal_the_binary(mg, golden, name):
    n, ip, _, _ = V.REF_CASES[name]
    assert np.array_equal(V.all_unknowns(n, ip), golden[name + "_idx"])
    assert np.array_equal(mg.vanka._all_cell_indices(np.asarray(n), mg.getVankaBlockSize(np.asarray(n), ip)[1], ip), golden[name + "_idx"])


@pytest.mark.parametrize("name", list(V.REF_CASES))
def test_restatement_reproduces_the_primitives(mg, golden, name):
    n, ip, cx, _ = V.REF_CASES[name]
    A, x0, b, D = V.ref_inputs(mg, name)
    x1 = V.restate_relax(A, x0.copy(), b, D, 1, n, ip, V.FULL_VANKA_RB)
    x3 = V.restate_relax(A, x1.copy(), b, D, 2, n, ip, V.FULL_VANKA_RB)
    for got, key in ((x1, "_x1"), (x3, "_x3")):
        ref = golden[name + key]
        e = np.abs(got - ref).max() / np.abs(ref).max()
        print(name, key, e)
        assert e <= TOL
    assert np.linalg.norm(b - A @ x3) < np.linalg.norm(b - A @ x0)      # the relaxation does relax
