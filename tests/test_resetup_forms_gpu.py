"""-m gpu: every value-dependent operator form after replaceMatrixInHierarchy on a resident FP64 handle, row by row.

mg_rap_FP64 recomputes the relaxation vectors and the Galerkin products in HBM and rebuilds what is derived from the values
(refresh_rowclasses, derive_class_d, build_staged, build_small27, build_band27, band_refill).  Small grids with the thresholds
lowered as tests/test_four_stage.py and tests/test_march27.py do it, so that the forms of the production sizes serve them:
  RC  Poisson on [33, 25, 15] and [23, 23, 23] cells - row-class forms on level 1, 27-point classes below;
  VB  div sigma grad on [33, 25, 15] (band_min_rows = 0) - the band form on level 1, band-27 below;
  SM  Poisson on [16, 16, 16] with default options - the small-level kernels;
  SA  SA_AMGsetup on anisotropic_divsiggrad([16] * 3) with SPAI and longrow_min_avg lowered.
Transitions, each through mg.replaceMatrixInHierarchy with p.device asserted to be the same object afterwards:
  T1 values x 1.75 (the classes stay);  T2 variable values on the same pattern (operator_rowclasses(1, A)[0] == 0 afterwards);
  T3 a new sigma (symmetric), then one stored upper entry changed (band_form's symmetric reads against (A != A.T).nnz == 0);
  T4 constant-coefficient values on the variable pattern;  T5 six rows changed, then six others;  T6 a new anisotropy (SA);
  T2 once more with coarseDeviceInverse=True (no mg_finalize runs after the refresh).
After every transition (_after): the device's operators equal the host mirror bit for bit; every coarse operator entry by entry
against the long-double Galerkin sum formed from the device's own finer level (tests/rap_crafted_cases.py: Terms, reference,
gamma(m + 2) sum|t|; coarse rows in blocks, none left out); every relaxation vector bit for bit (check_relax); on every level
l < L the residual, the sweep, alpha A x + beta y, P xc, R x and the two-stage pass row by row on guarded buffers with both input
families (tests/test_default_paths_families.py: _check_level); a solve of two steps - one cycle from zero, one from an iterate -
against the C oracle on the refreshed host hierarchy at 1e-10; then three columns are set on the handle and the residual, the
sweep, alpha A X + beta Y, P Xc and R X of every level are checked with check_block column by column (_blocks_after).  What
served each level is printed (_observed).
Sequences against a twin param that never went to the device (host path): transposeHierarchy then the replacement, and the
replacement then transposeHierarchy, on the non-symmetric operator of tests/test_transpose_device.py - equal patterns, values
within the entry bound on both sides right after the replacement (gamma(m + 2) sum|t|, each side from its own finer level; after a
transpose Ps[l] = Rs[l]' by the reference's literal assignments, so As[l+1] is no longer Rs As Ps and the device's values are compared
with the host mirror bit for bit instead), the solve at 1e-10, doTranspose == 0 after a replacement.
Blocks (test_rc_refresh_with_a_block_of_right_hand_sides): nrhs 3 and 4 set on the handle (adjustMemoryForNumRHS) BEFORE the
refresh, under coarseDeviceInverse=True, so that no mg_finalize runs afterwards; T1 (the lane SpMM kernels read the refreshed
dictionary of A) and T2 (A falls to csr_stream_spmm, P stays on the lane kernel); residual, sweep, alpha A X + beta Y, P Xc
and R X of every level with check_block column by column; then the single-vector checks on the same handle.
ComplexF64 (test_complex_adjoint_then_replacement): adjointHierarchy on the resident handle, then a replacement on the flipped
pattern, against a twin on the host path: equal patterns, every entry on both sides within the complex entry bound, the vectors
bit for bit, doTranspose == 0, the solve against the complex oracle at 1e-10."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import rap_crafted_cases as K
from oracle import mg_oracle as orc
from default_paths_check import Guarded, check_block
from test_default_paths_families import (_block_inputs, _block_out, _check_level, _inputs, _mesh, _observed, _scaled_normal, _smooth,
                                         _solve_check)

pytestmark = pytest.mark.gpu

ENV = {"MG_ROWCLASS_MIN_ROWS": "0", "MG_NO_SMALL": "1", "MG_MARCH_MIN_WG": "0", "MG_MARCH27_MIN_ROWS": "0", "MG_BAND_MIN_ROWS": "0"}
BLOCK_TERMS = 3_000_000          # terms of the long-double reference formed at a time


@pytest.fixture
def env(monkeypatch):
    def use(extra=None, defaults=False):
        for k in list(os.environ):
            if k.startswith("MG_"):
                monkeypatch.delenv(k)
        for k, v in ({} if defaults else ENV).items():
            monkeypatch.setenv(k, v)
        for k, v in (extra or {}).items():
            monkeypatch.setenv(k, v)
    return use


def _entries(tag, R, A, P, Cm):
    """Every entry of Cm against the long-double sum of its terms r a p within gamma(m + 2) sum|t|; coarse rows in blocks."""
    for M in (R, A, P, Cm):
        assert M.has_sorted_indices
    Ap, Pp = K.Pattern.of(A), K.Pattern.of(P)
    cost = np.asarray(abs(R).sign() @ (abs(A).sign() @ np.diff(P.indptr).astype(np.float64))).ravel()
    share, r0, n = 0.0, 0, R.shape[0]
    while r0 < n:
        r1 = r0 + 1
        acc = cost[r0]
        while r1 < n and acc + cost[r1] <= BLOCK_TERMS:
            acc += cost[r1]
            r1 += 1
        Rs, Cs = R[r0:r1], Cm[r0:r1]
        T = K.Terms(K.Pattern.of(Rs), Ap, Pp, K.Pattern.of(Cs))
        share = max(share, K.check_entries(f"{tag} rows {r0}..{r1}", "float64", T, Cs.data, K.reference(T, Rs.data, A.data, P.data)))
        r0 = r1
    return share


def _after(mg, tag, p, h, kind, omega, families=("a", "b"), blocks=3):
    from multigrid_jl_amd import device as D
    L = len(p.As)
    assert p.device is h and p.doTranspose == 0
    shares = []
    for l in range(1, L + 1):
        assert np.array_equal(h.get_values(l, D.MG_OP_A), p.As[l - 1].data), (tag, l)
    for l in range(1, L):
        R, A, P, Cm = p.Rs[l - 1], p.As[l - 1], p.Ps[l - 1], p.As[l]
        shares.append(_entries(f"{tag} As[{l + 1}]", R, A, P, Cm))
        d = np.asarray(p.relaxPrecs[l - 1], dtype=np.float64)
        K.check_relax(f"{tag} relaxPrecs[{l}]", "float64", kind, K.Pattern.of(A), A.data, d, omega)
        for fam in families:
            rng = np.random.default_rng((17 if fam == "a" else 29) + l)
            x, b = _inputs(fam, rng, A, _mesh(p, l))
            xc = _scaled_normal(rng, P.shape[1]) if fam == "a" else _smooth(P.shape[1], _mesh(p, l + 1))
            _check_level(h, f"{tag} level {l} ({fam})", l, A, d, P, R, x, b, xc, rng)
    _solve_check(mg, p)
    assert p.device is h
    if blocks:                       # the block handles, column by column: `blocks` columns set on the handle, then one again
        mg.adjustMemoryForNumRHS(p, blocks)
        assert p.device is h and h.nrhs == blocks
        _blocks_after(h, p, tag, blocks)
        mg.adjustMemoryForNumRHS(p, 1)
        assert p.device is h and h.nrhs == 1
    print(f"\n{tag}: rows {[a.shape[0] for a in p.As]}, largest share of an entry bound per level {[round(s, 3) for s in shares]}\n"
          + "\n".join(f"    {row!r}," for row in _observed(h, p)) + f"\n    four-stage form of level 1: {h.four_stage_form(1)[0]}")
    return shares


def _gmg(mg, A, mesh, levels, relax="Jac", omega=0.8, **kw):
    p = mg.getMGparam(np.float64, np.int64, levels, 8, 2, 0.0, relax, omega, 2, 1, "V", "NoMUMPS", 0.5, 0.0, **kw)
    mg.MGsetup(A, mesh, p)
    return p


def _variable(A, seed):
    """Variable values on A's pattern: the entries scaled symmetrically by a seeded field (diagonally dominant as A is)."""
    s = np.exp(0.3 * np.random.default_rng(seed).standard_normal(A.shape[0]))
    B = (sp.diags(s) @ A @ sp.diags(s)).tocsr()
    B.sort_indices()
    assert np.array_equal(B.indptr, A.indptr) and np.array_equal(B.indices, A.indices)
    return B


def _sigma_matrix(mg, mesh, cells, seed):
    sigma = np.exp(np.random.default_rng(seed).standard_normal(int(np.prod(cells))))
    A = mg.getNodalDivSigGradMatrix(mesh, sigma)
    A = (A + 1e-3 * abs(A).sum(axis=0).max() * sp.identity(A.shape[0], format="csr")).tocsr()
    A = ((A + A.T) * 0.5).tocsr()
    A.sort_indices()
    return A


@pytest.mark.parametrize("cells", [[33, 25, 15], [23, 23, 23]])
def test_rc_scaled_then_variable_then_exception_rows(mg, built, env, cells):
    """RC: T1, T5, T2 in this order on one resident handle."""
    from multigrid_jl_amd import device as D
    env()
    A, mesh = mg.poisson_shifted(cells)
    p = _gmg(mg, A, mesh, 3)
    h = mg.to_device(p)
    try:
        nc0 = h.operator_rowclasses(1, D.MG_OP_A)[0]
        assert nc0 > 0
        mg.replaceMatrixInHierarchy(p, (A * 1.75).tocsr())                                   # T1
        assert h.operator_rowclasses(1, D.MG_OP_A)[0] == nc0
        nexc0 = h.operator_kernel_info(1, D.MG_OP_A)[1]
        _after(mg, f"RC {cells} T1", p, h, 0, 0.8)
        n = A.shape[0]
        for rows in (np.arange(6) * 37 + n // 3, np.arange(6) * 41 + n // 2):                # T5: six rows, then six others
            B = (A * 1.75).tocsr()
            for q, i in enumerate(rows):       # (no two of the six rows alike, none like any other row)
                B.data[B.indptr[i]:B.indptr[i + 1]] *= 1.0 + 0.01 * (q + 1) * (1 + np.arange(B.indptr[i + 1] - B.indptr[i]))
            mg.replaceMatrixInHierarchy(p, B)
            # each changed row (its values now unlike any other row's) is an exception row or a class of its own; the rest keep theirs
            nc, nexc = h.operator_rowclasses(1, D.MG_OP_A)[0], h.operator_kernel_info(1, D.MG_OP_A)[1]
            print(f"T5: classes {nc0} -> {nc}, exception rows {nexc0} -> {nexc}")
            assert nc >= nc0 and nexc >= nexc0 and (nc - nc0) + (nexc - nexc0) == 6, (nc0, nc, nexc0, nexc)
            _after(mg, f"RC {cells} T5 rows {rows[0]}..", p, h, 0, 0.8)
        mg.replaceMatrixInHierarchy(p, _variable(A, 3))                                      # T2
        assert h.operator_rowclasses(1, D.MG_OP_A)[0] == 0
        _after(mg, f"RC {cells} T2", p, h, 0, 0.8)
    finally:
        mg.clear_(p)


def test_rc_variable_values_with_the_coarsest_inverse_built_on_the_device(mg, built, env):
    """T2 under coarseDeviceInverse=True: Python calls no mg_finalize after the refresh."""
    from multigrid_jl_amd import device as D
    env()
    A, mesh = mg.poisson_shifted([23, 23, 23])
    p = _gmg(mg, A, mesh, 3, coarseDeviceInverse=True)
    h = mg.to_device(p)
    try:
        assert h._coarse_device_inverse and h.operator_rowclasses(1, D.MG_OP_A)[0] > 0
        mg.replaceMatrixInHierarchy(p, _variable(A, 5))
        assert h.operator_rowclasses(1, D.MG_OP_A)[0] == 0
        _after(mg, "RC coarseDeviceInverse T2", p, h, 0, 0.8)
    finally:
        mg.clear_(p)


def test_vb_new_sigma_then_one_entry_then_constant_coefficients(mg, built, env):
    """VB: T3 (two steps) and T4 on one resident handle."""
    env()
    cells = [33, 25, 15]
    mesh = mg.getRegularMesh([0.0, 1.0] * 3, cells)
    A = _sigma_matrix(mg, mesh, cells, 11)
    p = _gmg(mg, A, mesh, 3)
    h = mg.to_device(p)
    try:
        assert h.band_form(1)[0] == 1 and h.band_form(1)[2] == 1, h.band_form(1)
        B = _sigma_matrix(mg, mesh, cells, 12)                                              # T3, first step: still symmetric
        assert (B != B.T).nnz == 0
        mg.replaceMatrixInHierarchy(p, B)
        assert h.band_form(1)[0] == 1 and h.band_form(1)[2] == 1, h.band_form(1)
        _after(mg, "VB T3 new sigma", p, h, 0, 0.8)
        B2 = B.copy()                                                                       # T3, second step: one stored upper entry
        i = B.shape[0] // 2
        k = B2.indptr[i] + int(np.searchsorted(B2.indices[B2.indptr[i]:B2.indptr[i + 1]], i + 1))
        assert B2.indices[k] == i + 1
        B2.data[k] *= 1.5
        assert (B2 != B2.T).nnz > 0
        mg.replaceMatrixInHierarchy(p, B2)
        assert h.band_form(1)[0] == 1 and h.band_form(1)[2] == 0, h.band_form(1)
        _after(mg, "VB T3 one upper entry", p, h, 0, 0.8)
        Cc, _ = mg.poisson_shifted(cells)                                                    # T4: constant coefficients on the variable pattern
        Cc.sort_indices()
        assert np.array_equal(Cc.indptr, B.indptr) and np.array_equal(Cc.indices, B.indices)
        mg.replaceMatrixInHierarchy(p, Cc)
        # the operator was uploaded without row classes: the band form goes on serving it, on symmetric reads again
        from multigrid_jl_amd import device as D
        assert (Cc != Cc.T).nnz == 0 and h.band_form(1)[0] == 1 and h.band_form(1)[2] == 1, h.band_form(1)
        assert h.sweep_residual_form(1)[0] == 4 and h.operator_kernel_variant(1, D.MG_OP_A) == -1
        assert h.operator_rowclasses(1, D.MG_OP_A)[0] == 0
        _after(mg, "VB T4 constant coefficients", p, h, 0, 0.8)
    finally:
        mg.clear_(p)


def test_sm_small_level_kernels_follow_the_new_values(mg, built, env):
    """SM: default options on [16, 16, 16] cells; T1 then T2."""
    from multigrid_jl_amd import device as D
    env(defaults=True)
    A, mesh = mg.poisson_shifted([16, 16, 16])
    p = _gmg(mg, A, mesh, 3)
    h = mg.to_device(p)
    try:
        assert 8 in [h.operator_kernel_variant(l, D.MG_OP_A) for l in (1, 2, 3)]
        mg.replaceMatrixInHierarchy(p, (A * 1.75).tocsr())
        _after(mg, "SM T1", p, h, 0, 0.8)
        mg.replaceMatrixInHierarchy(p, _variable(A, 7))
        _after(mg, "SM T2", p, h, 0, 0.8)
    finally:
        mg.clear_(p)


def test_sa_amg_new_anisotropy(mg, built, env):
    """SA: T6 - the first SA-AMG hierarchy through the device re-setup; one level at least on csr_longrow_spmv with 16-bit columns."""
    from multigrid_jl_amd import device as D
    A, _ = mg.anisotropic_divsiggrad([16] * 3, weights=(1.0, 0.25, 0.0625))
    p = mg.getMGparam(np.float64, np.int64, 14, 8, 2, 0.0, "SPAI", 1.0, 1, 1, "V", "Julia", 0.4, 0.0)
    mg.SA_AMGsetup(A, p, True, 1)
    # longrow_min_avg lowered to the densest level's entries per row (the default, 1000, is for production sizes)
    env(defaults=True, extra={"MG_LONGROW_MIN_AVG": str(int(max(a.nnz / a.shape[0] for a in p.As[1:-1])))})
    h = mg.to_device(p)
    try:
        kinds = [tuple(h.operator_stream_kernel(l, D.MG_OP_A)[:3]) for l in range(1, len(p.As))]
        assert any(k[0] == 3 and k[2] == 1 for k in kinds), kinds
        B, _ = mg.anisotropic_divsiggrad([16] * 3, weights=(0.5, 1.0, 0.125))
        assert np.array_equal(B.indptr, A.indptr) and np.array_equal(B.indices, A.indices)
        mg.replaceMatrixInHierarchy(p, B)
        _after(mg, "SA T6", p, h, 1, 1.0)
    finally:
        mg.clear_(p)


def _blocks_after(h, p, tag, nrhs):
    """Every block product of every level l < L, column by column (the calls of test_default_paths_families.py's block check)."""
    import torch
    from multigrid_jl_amd import device as D
    rng = np.random.default_rng(61 + nrhs)
    for l in range(1, len(p.As)):
        A, P, R = p.As[l - 1], p.Ps[l - 1], p.Rs[l - 1]
        d = np.asarray(p.relaxPrecs[l - 1], dtype=np.float64)
        n, t = A.shape[0], f"{tag} level {l} nrhs {nrhs}"
        X = _block_inputs(A, _mesh(p, l), nrhs)
        B = A @ X
        noise = 1e-6 * rng.standard_normal(n)
        for j in range(nrhs):
            B[:, j] += np.roll(noise, 5 * j) * 2.0 ** (3 * j - 20)
        xg, bg = Guarded.block(n, nrhs, X, out=False), Guarded.block(n, nrhs, B, out=False)
        prods = {}
        out = Guarded.block(n, nrhs)
        h.fused_dev(l, D.MG_K_RESIDUAL, bg.v, xg.v, out.v, nrhs)
        check_block(f"{t} fused residual", "residual", _block_out(out, None), A, X, None, B=B, prods=prods)
        out = Guarded.block(n, nrhs)
        h.fused_dev(l, D.MG_K_SMOOTH, bg.v, xg.v, out.v, nrhs)
        check_block(f"{t} fused smooth", "sweep", _block_out(out, None), A, X, None, B=B, d=d, prods=prods)
        for alpha, beta in ((0.5, -2.0), (1.0, 0.0)):
            out = Guarded.block(n, nrhs)
            if beta != 0.0:
                out.v.copy_(torch.from_numpy(np.ascontiguousarray(B).ravel()))
            h.spmv_dev(l, D.MG_OP_A, alpha, xg.v, beta, out.v, nrhs)
            check_block(f"{t} A spmm ({alpha}, {beta})", "spmv", _block_out(out, None), A, X, None, alpha=alpha, beta=beta, Y0=B, prods=prods)
        Xc = _block_inputs(P, _mesh(p, l + 1), nrhs)
        xcg = Guarded.block(P.shape[1], nrhs, Xc, out=False)
        out = Guarded.block(n, nrhs)
        out.v.copy_(torch.from_numpy(np.ascontiguousarray(B).ravel()))
        h.spmv_dev(l, D.MG_OP_P, 1.0, xcg.v, 1.0, out.v, nrhs)
        check_block(f"{t} P spmm (1, 1)", "spmv", _block_out(out, None), P, Xc, None, alpha=1.0, beta=1.0, Y0=B)
        out = Guarded.block(R.shape[0], nrhs)
        h.spmv_dev(l, D.MG_OP_R, 1.0, xg.v, 0.0, out.v, nrhs)
        check_block(f"{t} R spmm (1, 0)", "spmv", _block_out(out, None), R, X, None)
        for g in (xg, bg, xcg):
            g.host_guards()


@pytest.mark.parametrize("nrhs", [3, 4])
def test_rc_refresh_with_a_block_of_right_hand_sides(mg, built, env, nrhs):
    """T1 and T2 with nrhs columns on the handle and coarseDeviceInverse=True: nothing finalizes the handle after the refresh."""
    from multigrid_jl_amd import device as D
    env(extra={"MG_NO_COLUMNS": "1"})            # (blocks by the SpMM kernels, not column by column: read when the handle is created)
    A, mesh = mg.poisson_shifted([23, 23, 23])
    p = _gmg(mg, A, mesh, 3, coarseDeviceInverse=True)
    h = mg.to_device(p)
    try:
        assert h._coarse_device_inverse
        mg.adjustMemoryForNumRHS(p, nrhs)
        assert p.device is h and h.nrhs == nrhs
        lane = lambda w: h.operator_stream_kernel(1, w)[0] in (5, 6)
        for name, new, classes in (("T1", (A * 1.75).tocsr(), True), ("T2", _variable(A, 9), False)):
            mg.replaceMatrixInHierarchy(p, new)
            assert p.device is h and h.nrhs == nrhs
            kern = [tuple(h.operator_stream_kernel(l, w)[:2]) for l in (1, 2) for w in (D.MG_OP_A, D.MG_OP_P, D.MG_OP_R)]
            print(f"\nRC blocks {name} nrhs {nrhs}: (A, P, R) of levels 1, 2 served by {kern}")
            assert (h.operator_rowclasses(1, D.MG_OP_A)[0] > 0) == classes and lane(D.MG_OP_A) == classes
            assert lane(D.MG_OP_P)          # (P's dictionary does not change; R of these small grids is streamed: printed above)
            _blocks_after(h, p, f"RC blocks {name}", nrhs)
        mg.adjustMemoryForNumRHS(p, 1)
        assert p.device is h
        _after(mg, f"RC blocks nrhs {nrhs}, back to one column", p, h, 0, 0.8)
    finally:
        mg.clear_(p)


@pytest.mark.parametrize("relax", ["Jac", "SPAI"])
def test_complex_adjoint_then_replacement(mg, built, env, relax):
    import copy
    from complex_adjoint_cases import base_param
    from complex_cases import complex_rhs
    from test_complex_adjoint_gpu import _solve_matches_oracle
    env(defaults=True)
    p, A, _ = base_param(mg, relax, maxIter=2, tol=0.0)
    b = complex_rhs(A.shape[0], 9)
    try:
        dev = mg.to_device(p)
        mg.adjointHierarchy(p)
        assert p.device is dev and p.doTranspose == 1
        rng = np.random.default_rng(8)
        At = p.As[0]
        A2 = At.copy()
        A2.data = At.data * ((1.0 + 0.3 * rng.random(At.nnz)) + 0.2j * rng.random(At.nnz))
        A2 = (A2 + sp.diags(np.abs(At.diagonal()).max() * (0.5 + rng.random(At.shape[0])) * (1.0 + 0.25j))).tocsr()
        A2.sort_indices()
        assert np.array_equal(A2.indptr, At.indptr) and np.array_equal(A2.indices, At.indices)
        twin = copy.copy(p)
        twin.device, twin.LU = None, None
        twin.As, twin.Ps, twin.Rs = [M.copy() for M in p.As], list(p.Ps), list(p.Rs)
        twin.relaxPrecs = [np.array(d, copy=True) for d in p.relaxPrecs]
        mg.replaceMatrixInHierarchy(twin, A2)
        mg.replaceMatrixInHierarchy(p, A2)
        assert p.device is dev and twin.device is None and p.doTranspose == 0 and twin.doTranspose == 0
        kind = 1 if relax == "SPAI" else 0
        for l in range(1, len(p.As)):
            assert np.array_equal(p.As[l].indptr, twin.As[l].indptr) and np.array_equal(p.As[l].indices, twin.As[l].indices)
            for prm, who in ((p, "device"), (twin, "twin")):
                R, Af, P, Cm = prm.Rs[l - 1], prm.As[l - 1], prm.Ps[l - 1], prm.As[l]
                assert not np.iscomplexobj(R.data) and not np.iscomplexobj(P.data) and all(M.has_sorted_indices for M in (R, Af, P, Cm))
                T = K.Terms(K.Pattern.of(R), K.Pattern.of(Af), K.Pattern.of(P), K.Pattern.of(Cm))
                # the device adds its group copies at the end; scipy's product forms full complex products in another order: the
                # same count of roundings per path covers both (m + groups + 1 with the groups the device used)
                g = K.lane_groups(0, K.RAP_CAP, np.diff(Cm.indptr).max())
                share = K.check_entries(f"{who} As[{l + 1}]", "complex128", T, Cm.data, K.reference(T, R.data, Af.data, P.data), groups=g)
                print(f"\ncomplex {relax} {who} As[{l + 1}]: largest share of an entry bound {share:.3f}")
            assert np.array_equal(dev.get_values(l + 1, mg.device.MG_OP_A), p.As[l].data)
            K.check_relax(f"device relaxPrecs[{l}]", "complex128", kind, K.Pattern.of(p.As[l - 1]), p.As[l - 1].data,
                          np.asarray(p.relaxPrecs[l - 1]), 0.8)
        _solve_matches_oracle(mg, p, b, f"{relax} adjoint, then replaced")
        assert p.device is dev
    finally:
        mg.clear_(p)


def _nonsymmetric(mg, cells):
    A, mesh = mg.poisson_shifted(cells)
    n = A.shape[0]
    A = (A + sp.diags([np.linspace(0.05, 0.3, n - 1)], [1], format="csr") * abs(A[0, 0]) * 0.2).tocsr()
    A.sort_indices()
    return A, mesh


def _against_twin(mg, p, q):
    """p went through the device, q (the twin) through the host path: patterns equal, values within the entry bound on both sides."""
    for l in range(1, len(p.As)):
        a, b = p.As[l], q.As[l]
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
        bounds = []
        for prm in (p, q):                                   # each side against the long-double sum of its own finer level
            T = K.Terms(K.Pattern.of(prm.Rs[l - 1]), K.Pattern.of(prm.As[l - 1]), K.Pattern.of(prm.Ps[l - 1]), K.Pattern.of(prm.As[l]))
            ref = K.reference(T, prm.Rs[l - 1].data, prm.As[l - 1].data, prm.Ps[l - 1].data)
            K.check_entries(f"{'device' if prm is p else 'twin'} As[{l + 1}]", "float64", T, prm.As[l].data, ref)
            bounds.append(K.bound("float64", T, ref))
        if l == 1:                                           # the same fine operator on both sides: the two sums of the same terms
            assert p.As[0].data.tobytes() == q.As[0].data.tobytes() and (np.abs(a.data - b.data) <= bounds[0] + bounds[1]).all()


def _solve_against_twin(mg, p, q, h):
    """At the end of a sequence: equal patterns, the device's values are the host mirror's bit for bit, the solve matches the oracle
    on the twin at 1e-10."""
    from multigrid_jl_amd import device as D
    for l in range(len(p.As)):
        assert np.array_equal(p.As[l].indptr, q.As[l].indptr) and np.array_equal(p.As[l].indices, q.As[l].indices)
        assert np.array_equal(h.get_values(l + 1, D.MG_OP_A), p.As[l].data)
    b = mg.seeded_rhs(p.As[0])
    x, xo, hist = np.zeros_like(b), np.zeros_like(b), {}
    mg.solveMG(p, b, x)
    orc.solveMG(q, b, xo, False, hist)
    assert np.abs(p.resvec - hist["resvec"]).max() <= 1e-10 * hist["resvec"][0] and np.abs(x - xo).max() <= 1e-10 * np.abs(xo).max()


@pytest.mark.parametrize("order", ["transpose, replace", "replace, transpose"])
def test_sequences_against_a_twin_on_the_host_path(mg, built, env, order):
    env(defaults=True)
    A, mesh = _nonsymmetric(mg, [16, 12, 10])
    B = sp.csr_matrix((A.data * (1.0 + 0.2 * np.random.default_rng(4).random(A.nnz)), A.indices, A.indptr), shape=A.shape)
    p, q = _gmg(mg, A, mesh, 3), _gmg(mg, A, mesh, 3)
    h = mg.to_device(p)
    try:
        assert q.device is None
        for step in order.split(", "):
            for prm in (p, q):
                if step == "transpose":
                    mg.transposeHierarchy(prm)
                else:
                    new = B if prm.doTranspose == 0 else sp.csr_matrix(B.T)
                    new.sort_indices()
                    mg.replaceMatrixInHierarchy(prm, new)
                    assert prm.doTranspose == 0
            assert p.device is h and q.device is None
            if step == "replace":        # (after a transpose Ps[l] = Rs[l]' by the reference's literal assignments: As[l+1] is no longer Rs As Ps)
                _against_twin(mg, p, q)
        _solve_against_twin(mg, p, q, h)
        assert p.device is h
    finally:
        mg.clear_(p)
        mg.clear_(q)
