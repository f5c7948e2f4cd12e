"""-m gpu: the kernels the library picks for itself (no MG_* switch set) at production grid sizes, every product row by row.

Shapes: S1 400^3 cells (7 levels), S2 400x256x80 (7), S3 255x200x160 (even node count along x, 7), S4 2-D 4095x2048 (8).

The kernel tests of the other modules lower the size thresholds of MG_OPTIONS (csrc/mg_types.inc) and force the geometry on
grids of ~100 000 rows; here the thresholds and the cost model decide.  For each shape: (1) which kernel serves which level
(a literal table: a threshold that moves makes a shape fail here instead of quietly testing something else); (2) every
device product of every level against a long-double CSR reference, row by row (tests/default_paths_check.py), on NaN-filled
outputs between guard zones; (3) two solveMG steps (S1: also an early stop) against the C/OpenMP oracle."""
import os

import numpy as np
import pytest

from default_paths_check import Guarded, Product, check_residual, check_spmv, check_sweep, check_xpdr, norm_ld
from oracle import c_oracle

pytestmark = pytest.mark.gpu

SHAPES = {"S1": ([400, 400, 400], 7), "S2": ([400, 256, 80], 7), "S3": ([255, 200, 160], 7), "S4": ([4095, 2048], 8)}

# Per level l = 1..L: (variant of A, of P, of R, sweep_residual_form(l)[0], band_form(l)[0], profile keys of two solveMG steps).
# Variants (operator_kernel_variant): -1 streaming CSR, 1 csr_rowclass_window_spmv, 2 csr_rowclass_tile_spmv, 3 csr_rowclass_march_spmv,
# 4 csr_rowclass_lane_spmv, 7 marchr, 8 the small-level kernels (mg_small.hpp), 9 band-27, 10 grid_cell_prolong, 11 grid_wave_restrict;
# None: no such operator (coarsest level).  Forms: 0 two launches, 3 csr_rowclass_march3_spmv, 5 csr_rowclass_march27_spmv.
# Profile keys name what a variant does not: "restrict" without "residual" on a small level is the fused residual + restriction
# (grid27_small_resid_restrict), "smooth+prolong" the fused prolongation + first post-sweep; no "dscale" on a form-5 level: its
# pair from x = 0 forms x1 = d.*b itself.
# Thresholds (MG_OPTIONS): rowclass_min_rows 1e5, march27_min_rows 5e5, small_max_rows 3e5; the grid transfers of a vertex-centred
# pair (fine = 2 coarse - 1 nodes in every direction) take grid_cell_prolong / grid_wave_restrict at ANY size, ahead of marchr
# (marchr_min_rows 1e6 coarse rows) and the small transfer kernels - marchr (7) therefore serves no level of these shapes: it is
# built only for such pairs, where the wavefront form is chosen first.  A pair with an even node count is none of that (lane or
# streaming kernels), and the Galerkin operators below it vary from row to row (no small-level records: band-27).
_F1 = ("four-stage", "norm", "prolong", "restrict", "smooth+residual", "smooth+residual+norm")   # a 7-point fine level of 2 steps
_M27 = ("prolong", "restrict", "smooth", "smooth+residual")
_SMF = ("restrict", "smooth", "smooth+prolong")
_TWO = ("prolong", "residual", "restrict", "smooth")
EXPECTED = {
    # 401^3 -> 201^3 -> 101^3 -> 51^3 -> 26^3 -> 14^3 -> 8^3 nodes
    "S1": [(3, 10, 11, 3, 0, _F1),      # 64.5 M rows >= rowclass_min_rows: marching sweep, 2-D tile pair; odd pair: cell / wave transfers
           (2, 10, 11, 5, 0, _M27),     # 8.1 M >= march27_min_rows: the 27-point marching pair (from zero in a V-cycle)
           (2, 10, 11, 5, 0, _M27),     # 1.03 M >= march27_min_rows
           (4, 10, 11, 0, 0, _SMF),     # 132 651: row classes (>= rowclass_min_rows) below march27_min_rows; <= small_max_rows: fused small launches
           (8, -1, -1, 0, 0, _TWO),     # 17 576 < rowclass_min_rows: small kernels; 26 nodes (even): no vertex-centred pair below
           (9, -1, -1, 0, 2, _TWO),     # Galerkin product through the even pair: band-27
           (9, None, None, None, None, ("coarse",))],
    # 401x257x81 -> 201x129x41 -> 101x65x21 -> 51x33x11 -> 26x17x6 -> 14x9x4 -> 8x5x3
    "S2": [(3, 10, 11, 3, 0, _F1),      # 8.3 M rows: as S1's fine level
           (2, 10, 11, 5, 0, _M27),     # 1.06 M >= march27_min_rows, partial tiles in y and z
           (4, 10, 11, 0, 0, _SMF),     # 137 865: row classes below march27_min_rows, fused small launches
           (8, 10, 11, 0, 0, _SMF),     # 18 513 < rowclass_min_rows: small kernels; odd pair: cell / wave transfers
           (8, -1, -1, 0, 0, _TWO),     # 26x17x6: even counts, no vertex-centred pair below
           (9, -1, -1, 0, 2, _TWO),
           (9, None, None, None, None, ("coarse",))],
    # 256x201x161 (even along x) -> 129x101x81 -> 65x51x41 -> 33x26x21 -> 17x14x11 -> 9x8x6 -> 5x5x4
    "S3": [(3, 4, 4, 3, 0, _F1),        # 8.3 M rows: the marching forms; even x: no cell / wave / marchr transfers - the lane kernel, visibly
           (2, 10, 11, 5, 0, _M27),     # 1.06 M >= march27_min_rows
           (9, 10, 11, 0, 2, _TWO),     # 135 915: rows differ (Galerkin through the even pair) - no row classes, band-27
           (9, -1, -1, 0, 2, _TWO),     # 26 nodes along y: no vertex-centred pair below
           (9, -1, -1, 0, 2, _TWO),
           (9, -1, -1, 0, 2, _TWO),
           (9, None, None, None, None, ("coarse",))],
    # 2-D: 4096x2049 (even along x) -> 2049x1025 -> 1025x513 -> 513x257 -> 257x129 -> 129x65 -> 65x33 -> 33x17: 9-point Galerkin levels
    "S4": [(1, 4, 4, 0, 0, ("dscale", "norm", "prolong", "residual", "restrict", "smooth")),   # 5-point, 8.4 M rows: windows; no 3-D marching form
           (1, 10, 11, 0, 0, _TWO),     # 2.1 M rows
           (4, 10, 11, 0, 0, _TWO),     # 526 k
           (4, 10, 11, 0, 0, _TWO),     # 132 k >= rowclass_min_rows
           (9, 10, 11, 0, 2, _TWO),     # 33 k < rowclass_min_rows: rows differ (even pair above) - band-27
           (9, 10, 11, 0, 2, _TWO),
           (9, 10, 11, 0, 2, _TWO),
           (9, None, None, None, None, ("coarse",))],
}
FOUR_STAGE = {"S1": True, "S2": True, "S3": True, "S4": False}      # four_stage_form(1)[0]: 3-D fine levels with the tile pair


def _clean_env(mp):
    for k in list(os.environ):
        if k.startswith("MG_"):
            mp.delenv(k)
    assert not [k for k in os.environ if k.startswith("MG_")]


@pytest.fixture(autouse=True)
def _defaults(monkeypatch):
    _clean_env(monkeypatch)


@pytest.fixture(scope="module", params=sorted(SHAPES))
def shape(request, mg, built):
    cells, levels = SHAPES[request.param]
    with pytest.MonkeyPatch.context() as mp:
        _clean_env(mp)          # (the handle reads its options from the environment when it is created)
        A, mesh = mg.poisson_shifted(cells)
        p = mg.getMGparam(np.float64, np.int64, levels, 8, 2, 0.0, "Jac", 0.8, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
        mg.MGsetup(A, mesh, p)
        assert len(p.As) == levels and min(int(v) for m in p.Meshes for v in m.n) >= 2     # every dimension keeps >= 3 nodes
        b = mg.seeded_rhs(A)
        h = mg.to_device(p)
        yield request.param, A, p, b, h
        mg.clear_(p)


def _variant(h, l, which):
    try:
        return h.operator_kernel_variant(l, which)
    except Exception:
        return None


def test_which_kernel_serves_each_level(mg, shape):
    from multigrid_jl_amd import device as D
    name, A, p, b, h = shape
    L = len(p.As)
    keep = (p.maxOuterIter, p.relativeTol)
    h.profile_enable(True)
    h.profile_reset()
    try:
        p.maxOuterIter, p.relativeTol = 2, 0.0
        mg.solveMG(p, b, np.zeros_like(b))
        prof = h.profile()
    finally:
        h.profile_enable(False)
        p.maxOuterIter, p.relativeTol = keep
    got = []
    for l in range(1, L + 1):
        got.append((_variant(h, l, D.MG_OP_A), _variant(h, l, D.MG_OP_P) if l < L else None, _variant(h, l, D.MG_OP_R) if l < L else None,
                    h.sweep_residual_form(l)[0] if l < L else None, h.band_form(l)[0] if l < L else None,
                    tuple(sorted(k for (lv, k) in prof if lv == l))))
    four = h.four_stage_form(1)[0]
    assert (got, four) == (EXPECTED[name], FOUR_STAGE[name]), f"{name}: observed\n{got!r}\nfour-stage {four}"


def _smooth_field(mesh):
    nodes = [int(v) + 1 for v in mesh.n]
    f = np.ones(1)
    for n in reversed(nodes):          # (x fastest: row = i + n1 (j + n2 k))
        f = np.multiply.outer(f, np.sin(np.pi * (np.arange(n) + 1.0) / (n + 1.0)) + 0.25 * np.cos(np.pi * np.arange(n) / n))
    return f.ravel()


def _scaled_normal(rng, n):
    return rng.standard_normal(n) * np.exp2(rng.integers(-8, 9, n)).astype(np.float64)


def _inputs(family, rng, A, mesh):
    """(x, b) of a level: (a) standard normal times 2^k, k uniform in [-8, 8]; (b) x a low-frequency field, b = A x + 1e-6 noise."""
    n = A.shape[0]
    if family == "a":
        return _scaled_normal(rng, n), _scaled_normal(rng, n)
    x = _smooth_field(mesh)
    return x, A @ x + 1e-6 * rng.standard_normal(n)


@pytest.mark.parametrize("family", ["a", "b"])
def test_level_products_row_by_row(mg, shape, family):
    import torch
    from multigrid_jl_amd import device as D
    name, _, p, _, h = shape
    L = len(p.As)
    rng = np.random.default_rng(17 if family == "a" else 29)
    for l in range(1, L):
        A, d, mesh = p.As[l - 1], np.asarray(p.relaxPrecs[l - 1], dtype=np.float64), p.Meshes[l - 1]
        n = A.shape[0]
        tag = f"{name} level {l} ({family})"
        x, b = _inputs(family, rng, A, mesh)
        xg, bg = Guarded(n, x, out=False), Guarded(n, b, out=False)
        pr = Product(A, x)
        out = Guarded(n)
        h.fused_dev(l, D.MG_K_RESIDUAL, bg.v, xg.v, out.v)
        check_residual(f"{tag} fused residual", out.host(), b, pr)
        out = Guarded(n)
        h.fused_dev(l, D.MG_K_SMOOTH, bg.v, xg.v, out.v)
        check_sweep(f"{tag} fused smooth", out.host(), x, d, b, pr)
        y0 = _scaled_normal(rng, n)
        for alpha, beta, init in ((-1.0, 1.0, b), (0.5, -2.0, y0), (1.0, 0.0, None)):
            out = Guarded(n)
            if init is not None:
                out.v.copy_(torch.from_numpy(init))
            h.spmv_dev(l, D.MG_OP_A, alpha, xg.v, beta, out.v)
            check_spmv(f"{tag} A spmv ({alpha}, {beta})", out.host(), alpha, pr, beta, init)
        # transfers: P (coarse -> fine, beta = 1) and R (fine -> coarse, beta = 0 on a NaN target)
        P, R = p.Ps[l - 1], p.Rs[l - 1]
        xc = _scaled_normal(rng, P.shape[1]) if family == "a" else _smooth_field(p.Meshes[l])
        xcg, y0 = Guarded(P.shape[1], xc, out=False), _scaled_normal(rng, n)
        out = Guarded(n)
        out.v.copy_(torch.from_numpy(y0))
        h.spmv_dev(l, D.MG_OP_P, 1.0, xcg.v, 1.0, out.v)
        check_spmv(f"{tag} P spmv (1, 1)", out.host(), 1.0, Product(P, xc), 1.0, y0)
        out = Guarded(R.shape[0])
        h.spmv_dev(l, D.MG_OP_R, 1.0, xg.v, 0.0, out.v)
        check_spmv(f"{tag} R spmv (1, 0)", out.host(), 1.0, Product(R, x))
        del out, xcg, pr
        # the two-stage pass: t from x, then r [and xn] from the device's t, ||r|| from the device's r (the 27-point form
        # serves the pair alone: t and r)
        form = h.sweep_residual_form(l)[0]
        if form != 0:
            t, r, xn = Guarded(n), Guarded(n), (Guarded(n) if form != 5 else None)
            nrm = h.sweep_residual_dev(l, bg.v, xg.v, t.v, r.v, xn.v if xn else None, form != 5)
            th, rh = t.host(), r.host()
            check_sweep(f"{tag} pass t", th, x, d, b, Product(A, x))
            check_residual(f"{tag} pass r", rh, b, Product(A, th))
            if form != 5:
                xnh = xn.host()
                check_xpdr(f"{tag} pass xn", xnh, th, d, rh)
                want = norm_ld(rh)
                assert abs(nrm - want) <= 1e-13 * want, (tag, nrm, want)
            if l == 1 and h.four_stage_form(1)[0]:
                _four_stage(h, tag, A, d, b, bg, xg, th, rh, xn, xnh, nrm)
        for g in (xg, bg):
            g.host_guards()


def _four_stage(h, tag, A, d, b, bg, xg, th, rh, xn, xnh, nrm):
    """four_stage_dev on level 1: tp, rp equal the two chained two-stage passes bit for bit; the second pass checked stage by
    stage (t2 from the device's xn, r2 from the device's t2); ||r|| of the first stage."""
    import torch
    n = A.shape[0]
    tp, rp = Guarded(n), Guarded(n)
    nrm4 = h.four_stage_dev(1, bg.v, xg.v, tp.v, rp.v)
    t2, r2 = Guarded(n), Guarded(n)
    h.sweep_residual_dev(1, bg.v, xn.v, t2.v, r2.v)
    tph, rph, t2h, r2h = tp.host(), rp.host(), t2.host(), r2.host()
    assert torch.equal(tp.v, t2.v) and torch.equal(rp.v, r2.v), tag
    check_sweep(f"{tag} second pass t2", t2h, xnh, d, b, Product(A, xnh))
    check_residual(f"{tag} four-stage rp", rph, b, Product(A, tph))
    want = norm_ld(rh)
    assert abs(nrm4 - want) <= 1e-13 * want, (tag, nrm4, want)


def test_solve_matches_c_oracle(mg, shape):
    name, A, p, b, h = shape
    x = np.zeros_like(b)
    mg.solveMG(p, b, x)
    co = c_oracle.COracle(p, 1)
    xo = np.zeros_like(b)
    it, rv = co.solveMG(b, xo, 0.0, 2, c_oracle.max_threads())
    assert it == 2 and len(p.resvec) == 3 and np.abs(rv - p.resvec).max() / rv[0] < 1e-10
    assert np.abs(x - xo).max() <= 1e-10 * np.abs(xo).max()
    assert abs(np.linalg.norm(b - A @ x) - p.resvec[-1]) <= 1e-10 * p.resvec[0]
    if name != "S1":
        return
    # the early stop: the loop ends part-way, the speculative four-stage step behind the stopping test is thrown away
    keep = (p.maxOuterIter, p.relativeTol)
    try:
        p.maxOuterIter, p.relativeTol = 6, 1e-3
        x = np.zeros_like(b)
        mg.solveMG(p, b, x)
        resvec = np.array(p.resvec)
    finally:
        p.maxOuterIter, p.relativeTol = keep
    xo = np.zeros_like(b)
    it, rv = co.solveMG(b, xo, 1e-3, 6, c_oracle.max_threads())
    assert 2 <= it < 6 and len(resvec) == it + 1, (it, len(resvec))
    assert np.abs(rv - resvec).max() / rv[0] < 1e-10
    assert np.abs(x - xo).max() <= 1e-10 * np.abs(xo).max()
    assert abs(np.linalg.norm(b - A @ x) - resvec[-1]) <= 1e-10 * resvec[0]


def test_each_default_kernel_serves_some_level():
    """Across S1-S4 (the table above, which the introspection test holds to what the device reports): the four-stage pass,
    the 27-point marching form, the small-level kernels with both fused small launches, the cell prolongation and the
    wavefront restriction each serve at least one level."""
    rows = [row for t in EXPECTED.values() for row in t]
    assert any(FOUR_STAGE.values()) and any("four-stage" in row[5] for row in rows)
    assert any(row[3] == 5 for row in rows)
    assert any(row[0] == 8 for row in rows)
    assert any("smooth+prolong" in row[5] for row in rows)
    assert any("restrict" in row[5] and "residual" not in row[5] and row[2] == 11 for row in rows)
    assert any(row[2] == 11 for row in rows) and any(row[1] == 10 for row in rows)
