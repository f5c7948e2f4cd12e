"""Host side of the coarsest solve by a solver object (param.LU a DomainDecompositionParam or a parallelJuliaSolver preset
before MGsetup: MGsetup.jl:323-331, MGcycle.jl:138-148, MGdef.jl:141-143, 200-201), the C ABI's new names, and the comparands
of tests/test_coarse_solver_gpu.py checked against a dense two-grid computation.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import complex_oracle as corc
import coarse_solver_cases as cs
from complex_cases import complex_rhs, helmholtz
from oracle import mg_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgvcycle.h")
NEW = ["mg_dd0_apply_FP64", "mg_dd0_apply_CFP64", "mg_dd0_apply_dev_FP64", "mg_dd0_apply_dev_CFP64", "mg_set_coarse_dd", "mg_coarse_form"]


def test_new_symbols_declared_exported_and_bound(mg, built):
    """Fails without the feature: the parent's header, library and binding have none of these."""
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\bint\s+(mg_\w+)\s*\(", header))
    lib = mg.device.load_library()
    for n in NEW:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in mg.device.SIGNATURES, n


@pytest.mark.parametrize("VAL", [np.float64, np.complex128])
def test_preset_dd_param_is_set_up_and_kept(mg, VAL):
    """Fails without the feature: defineCoarsestAinv overwrote a preset LU with a SuperLU factor."""
    A, mesh = (mg.poisson_shifted([16, 16]) if VAL is np.float64 else helmholtz(mg, [16, 16], 0.5, 0.5))
    LU = cs.dd_lu(mg, mesh, [2, 2], [1, 1], VAL)
    p = cs.setup(mg, A, mesh, 2, LU, VAL)
    assert p.LU is LU
    assert len(LU.PrecParams) == 4 and len(LU.GlobalIndices) == 4
    assert LU.Mesh is p.Meshes[-1] and list(LU.Mesh.n) == [8, 8]
    assert all(q.Ainv.L is not None for q in LU.PrecParams)
    assert LU._handle is None and p.device is None              # nothing touched a device


@pytest.mark.parametrize("VAL", [np.float64, np.complex128])
def test_preset_parallel_julia_solver_is_set_up_and_kept(mg, VAL):
    A, mesh = (mg.poisson_shifted([16, 16]) if VAL is np.float64 else helmholtz(mg, [16, 16], 0.5, 0.5))
    LU = cs.pjs_lu(mg, VAL)
    p = cs.setup(mg, A, mesh, 2, LU, VAL)
    assert p.LU is LU and LU.L is not None and LU.L.nnz > 0 and LU.L.shape == p.As[-1].shape
    Ac = p.As[-1].toarray()
    prod = (LU.L @ LU.U).toarray()
    assert np.abs(Ac[np.ix_(LU.p - 1, LU.q - 1)] - prod).max() <= 1e-12 * np.abs(prod).max()
    assert LU._handle is None


def test_parallel_julia_solver_under_sa_amg(mg):
    A, _ = mg.poisson_shifted([24, 24])
    p = mg.getMGparam(np.float64, np.int64, 3, 8, 5, 1e-8, "SPAI", 1.0, 1, 1, "V", "NoMUMPS", 0.5, 0.0)
    LU = cs.pjs_lu(mg)
    p.LU = LU
    mg.SA_AMGsetup(A, p, True, 1, False)
    assert p.LU is LU and LU.L is not None and LU.L.shape == p.As[-1].shape


def test_copy_solver_copies_a_solver_object(mg):
    A, mesh = mg.poisson_shifted([16, 16])
    LU = cs.dd_lu(mg, mesh, [2, 2], [1, 1])
    p = cs.setup(mg, A, mesh, 2, LU)
    q = mg.copySolver(p)
    assert isinstance(q.LU, mg.DomainDecompositionParam) and q.LU is not LU
    assert q.LU.numDomains == [2, 2] and q.LU.overlap == [1, 1] and len(q.LU.PrecParams) == 0     # the settings, not the setup
    assert q.LU.Ainv is not LU.Ainv and isinstance(q.LU.Ainv, mg.ParallelJuliaSolver.parallelJuliaSolver)
    assert len(q.As) == 0
    pj = cs.setup(mg, A, mesh, 2, cs.pjs_lu(mg))
    qj = mg.copySolver(pj)
    assert isinstance(qj.LU, mg.ParallelJuliaSolver.parallelJuliaSolver) and qj.LU is not pj.LU
    assert qj.LU.L is not pj.LU.L and (qj.LU.L != pj.LU.L).nnz == 0       # PJS.copySolver keeps a set-up solver set up
    plain = cs.setup(mg, A, mesh, 2, None)
    assert plain.LU is not None and mg.copySolver(plain).LU is None         # a plain factorisation is still not copied


@pytest.mark.parametrize("how", ["destroyCoarsestLU", "clear_"])
def test_destroy_keeps_and_clears_a_solver_object(mg, how):
    A, mesh = mg.poisson_shifted([16, 16])
    LU = cs.dd_lu(mg, mesh, [2, 2], [1, 1])
    p = cs.setup(mg, A, mesh, 2, LU)
    getattr(mg, how)(p)
    assert p.LU is LU and len(LU.PrecParams) == 0 and len(LU.GlobalIndices) == 0 and LU._handle is None
    assert LU.numDomains == [2, 2]
    LUj = cs.pjs_lu(mg)
    pj = cs.setup(mg, A, mesh, 2, LUj)
    getattr(mg, how)(pj)
    assert pj.LU is LUj and LUj.L is None
    plain = cs.setup(mg, A, mesh, 2, None)
    getattr(mg, how)(plain)
    assert plain.LU is None


def test_refusals_at_setup(mg):
    A, mesh = mg.poisson_shifted([24, 24])
    p = mg.getMGparam(np.float64, np.int64, 3, 8, 5, 1e-8, "SPAI", 1.0, 1, 1, "V", "NoMUMPS", 0.5, 0.0)
    p.LU = cs.dd_lu(mg, mesh, [2, 2], [1, 1])
    with pytest.raises(ValueError):
        mg.SA_AMGsetup(A, p, True, 1, False)                     # no meshes: the reference fails there too
    p = mg.getMGparam(np.float64, np.int64, 2, 8, 5, 1e-8, "Jac", 0.8, 2, 2, "V", "NoMUMPS", 0.5, 0.0)
    p.LU = cs.dd_lu(mg, mesh, [2, 2], [1, 1], np.complex128)
    with pytest.raises(TypeError):
        mg.MGsetup(A, mesh, p)
    p.LU = cs.pjs_lu(mg, np.complex128)
    with pytest.raises(TypeError):
        mg.MGsetup(A, mesh, p)


def test_replace_matrix_sets_the_object_up_again(mg):
    A, mesh = mg.poisson_shifted([16, 16])
    LU = cs.dd_lu(mg, mesh, [2, 2], [1, 1])
    p = cs.setup(mg, A, mesh, 2, LU)
    old = LU.PrecParams[0].Ainv.L.copy()
    mg.replaceMatrixInHierarchy(p, (2.0 * A).tocsr())
    assert p.LU is LU and len(LU.PrecParams) == 4
    new = LU.PrecParams[0].Ainv
    prod = (new.L @ new.U).toarray()
    I = LU.GlobalIndices[0].astype(np.int64) - 1
    sub = p.As[-1][I][:, I].toarray()
    assert np.abs(sub[np.ix_(new.p - 1, new.q - 1)] - prod).max() <= 1e-12 * np.abs(prod).max()
    assert old.shape == new.L.shape


def test_transpose_replaces_the_object_by_a_plain_factorisation(mg):
    A, mesh = mg.poisson_shifted([16, 16])
    LU = cs.dd_lu(mg, mesh, [2, 2], [1, 1])
    p = cs.setup(mg, A, mesh, 2, LU)
    mg.transposeHierarchy(p)
    assert p.LU is not LU and hasattr(p.LU, "solve") and hasattr(p.LU, "perm_r")     # MGsetup.jl:310-311: lu(sparse(AT'))
    assert len(LU.PrecParams) == 0                                                  # ... after destroyCoarsestLU cleared it


# ---- the comparands of the GPU tests against a dense two-grid computation (8^2 cells) ----------------------------------------
def _dense_sweep(mg, Ac, n_cells, boxes, overlap, b):
    """One multiplicative Schwarz sweep from zero with dense sub-domain solves: colours 1..4 (odd / even box index per
    dimension, the first dimension the slower bit), the boxes of a colour in linear order (first index fastest)."""
    x = np.zeros(Ac.shape[0], dtype=Ac.dtype)
    boxes_of = {c: [] for c in range(1, 5)}
    for j in range(1, boxes[1] + 1):
        for i in range(1, boxes[0] + 1):
            boxes_of[1 + 2 * (1 - i % 2) + (1 - j % 2)].append((i, j))
    for c in range(1, 5):
        for loc in boxes_of[c]:
            I = np.asarray(mg.getNodalIndicesOfCell(boxes, overlap, list(loc), np.asarray(n_cells)), dtype=np.int64) - 1
            x[I] += np.linalg.solve(Ac[np.ix_(I, I)], (b - Ac @ x)[I])
    return x


def _dense_two_grid(p, coarse, b, x0):
    """V(nu1, nu2) two-grid cycle with dense matrices: x' = x + d.*(b - A x) sweeps, coarse correction, sweeps."""
    A, P, R = p.As[0].toarray(), p.Ps[0].toarray(), p.Rs[0].toarray()
    d = p.relaxPrecs[0]
    x = x0.copy()
    for _ in range(max(1, p.relaxPre(1))):
        x = x + d * (b - A @ x)
    x = x + P @ coarse(R @ (b - A @ x))
    for _ in range(max(1, p.relaxPost(1))):
        x = x + d * (b - A @ x)
    return x


@pytest.mark.parametrize("VAL", [np.float64, np.complex128])
@pytest.mark.parametrize("kind", ["dd", "splu"])
def test_adapter_oracles_agree_with_dense_two_grid(mg, VAL, kind):
    cx = VAL is np.complex128
    A, mesh = helmholtz(mg, [8, 8], 0.5, 0.5) if cx else mg.poisson_shifted([8, 8])
    boxes, ov = [2, 2], [1, 1]
    LU = cs.dd_lu(mg, mesh, boxes, ov, VAL) if kind == "dd" else cs.pjs_lu(mg, VAL)
    p = cs.setup(mg, A, mesh, 2, LU, VAL)
    assert [M.shape[0] for M in p.As] == [81, 25]
    adapter = cs.SweepLU(mg, p, boxes, ov) if kind == "dd" else cs.SpluLU(p)
    q = cs.oracle_param(p, adapter)
    assert q.LU is adapter and p.LU is LU and q.As is p.As
    Ac = p.As[-1].toarray()
    coarse = (lambda r: _dense_sweep(mg, Ac, [4, 4], boxes, ov, r)) if kind == "dd" else (lambda r: np.linalg.solve(Ac, r))
    b = complex_rhs(81, 3) if cx else np.random.default_rng(3).standard_normal(81)
    for x0 in (np.zeros_like(b), (complex_rhs(81, 4) if cx else np.random.default_rng(4).standard_normal(81))):
        ref = _dense_two_grid(p, coarse, b, x0)
        x = x0.copy()
        x = corc.recursiveCycle(q, b, x, 1) if cx else orc.recursiveCycle(q, b, x, 1)
        err = cs.relmax(x, ref)
        print(f"{kind} {np.dtype(VAL)}: restatement against the dense two-grid cycle {err:.3e}")
        assert err <= 1e-12
