"""-m gpu: the row-by-row method of tests/test_default_paths.py on the operator families that module does not reach - variable
coefficients (band forms, pattern-coded CSR, band-27), general CSR (SA-AMG: csr_stream_spmv, csr_longrow_spmv, the SPAI vectors)
and blocks of right-hand sides (the lane SpMM kernels, csr_stream_spmm) - with no MG_* switch set and hierarchies built on the host.

Hierarchies: V1 div sigma grad on 256^3 cells (log-normal sigma, seed 11), V2 the same on 255x200x160 symmetrised entry by entry,
V3 = V2 with ONE stored upper entry of the fine operator changed (values replaced on the resident hierarchy, nothing rebuilt),
A1 / A2 SA-AMG on anisotropic diffusion (128^3 at 16:4:1, 64^3 at SURVEY's 1 : 1e-2 : 1e-4), SY a hand-assembled general-CSR
hierarchy (empty rows, rows that straddle and exceed an LDS chunk, a row spanning > 65 535 columns, row lengths that are multiples
of 64), C5 the Poisson 256^3 hierarchy (blocks only: its single-vector kernels are tests/test_default_paths.py's).

Per hierarchy: a literal table of what serves each level; every product of every level l < L row by row (both input families);
the solve against the C/OpenMP oracle; for A1 / A2 the level sizes, literally, and every SPAI vector against long double.

Blocks (C5, V1, A1, SY; nrhs 3 and 16): the device-resident entry points take a block as [row][column] (entry (i, j) at i * nrhs + j; the
host entry points transpose a column-major host block into that) - Guarded.block.  Inputs are family (b) in every column (the time the
long-double references take allows one family here), column j shifted by 13 j rows and scaled by 2^(3j - 20); column 1 is zero (not
the last column of an odd block).  Every column of every level is checked against its own long-double product, except on a first
level of more than 4 M rows with 16 columns: there the references are those of columns {0, 1, 2, 7, 14, 15} and the other columns
must hold no NaN (the single-vector kernels and the block kernels are nowhere documented to sum a row in the same order, so those
columns are not compared with them)."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import default_paths_check as C
from default_paths_check import (LD, Guarded, Product, check_block, check_residual, check_spmv, check_sweep, check_xpdr, gamma,
                                 norm_ld)
from oracle import c_oracle

pytestmark = pytest.mark.gpu

GMG = {"V1": [256, 256, 256], "V2": [255, 200, 160], "C5": [256, 256, 256]}
SA = {"A1": ([128] * 3, (1.0, 0.25, 0.0625), 2), "A2": ([64] * 3, (1.0, 1e-2, 1e-4), 3)}      # cells, edge weights, solveMG steps
# which checks run on which hierarchy (the classes at the end of the module: one per hierarchy, built once, tests grouped by it)
SINGLE = ["V1", "V2", "A1", "A2", "SY"]
SOLVED = ["V1", "V2", "A1", "A2"]
BLOCKS = ["C5", "V1", "A1", "SY"]        # (SY: csr_stream_spmm on empty rows and on a row longer than its 1024-entry chunk)

# Host-built hierarchies are deterministic: a setup change that alters the aggregation fails here.
LEVEL_ROWS = {"A1": [2146689, 744484, 186613, 37429, 6586, 1115, 199, 39],
              "A2": [274625, 96694, 35655, 11807, 3301, 945, 373, 313, 312, 1]}
LEVEL_NNZ = {"A1": [14926977, 38992928, 82676511, 101788009, 30080760, 1243225, 39601, 1521],
             "A2": [1897025, 4909470, 18703653, 41272289, 10851207, 893025, 139129, 97969, 97344, 1]}

# Per level l = 1..L-1: (variant of A, of P, of R [operator_kernel_variant: -1 streaming formats, 9 band-27, 10 grid_cell_prolong,
# 11 grid_wave_restrict, 8 small-level kernels], stream kernel of A, of P, of R [operator_stream_kernel()[:3]: (kernel, NT, 16-bit
# columns); kernel 0 none, 1 csr_pattern_spmv, 2 csr_stream_spmv, 3 csr_longrow_spmv], sweep_residual_form(l)[0] [4: band form],
# (band_form(l)[0], [2], [3]) = (1 band / 2 band-27, symmetric reads, value planes streamed)).
# Thresholds (MG_OPTIONS, csrc/mg_types.inc): band_min_rows 1e5, band27_max_rows 4e7, longrow_min_avg 1000 entries per row on average;
# NT (non-temporal matrix loads) where 12 B x nnz > 128 MB.
_Z = (0, 0, 0)
_B27 = (9, 10, 11, _Z, _Z, _Z, 0, (2, 0, 27))     # Galerkin level of a vertex-centred pair: band-27, cell prolongation, wavefront restriction
EXPECTED = {
    # 257^3 -> 129^3 -> 65^3 -> 33^3 -> 17^3 -> 9^3 nodes
    "V1": [(-1, 10, 11, (1, 1, 0), _Z, _Z, 4, (1, 1, 4)),   # 17.0 M rows, no two rows equal: no row classes; >= band_min_rows: the band form serves the
                                                            # two-stage pass, csr_pattern_spmv (7-point patterns, 119 M non-zeros: NT) the single
                                                            # products.  SYMMETRIC reads (4 of 7 planes): scipy's G' diag(sigma) G + shift is
                                                            # symmetric bit for bit (the device's band_sym_check finds no differing pair)
           _B27, _B27, _B27, _B27],                         # 27-point Galerkin levels <= band27_max_rows: band-27 at every size, FULL reads (27 planes):
                                                            # R A P is symmetric only up to rounding, and band_sym_tol is off by default
    # 256x201x161 (even along x) -> 129x101x81 -> 65x51x41 -> 33x26x21 -> 17x14x11 -> 9x8x6 -> 5x5x4
    "V2": [(-1, 4, 4, (1, 1, 0), _Z, _Z, 4, (1, 1, 4)),     # 8.3 M rows: as V1 (symmetrised explicitly); even x: the lane kernel for P and R
           _B27, _B27,                                      # 1.06 M and 135 915 rows
           (9, -1, -1, _Z, (2, 0, 0), (1, 0, 0), 0, (2, 0, 27)),   # 26 nodes along y: no vertex-centred pair below - P streamed, R pattern-coded
           (9, -1, -1, _Z, (2, 0, 0), (1, 0, 0), 0, (2, 0, 27)),
           (9, -1, -1, _Z, (2, 0, 0), (1, 0, 0), 0, (2, 0, 27))],
    # V2's first level after one stored entry changed (test_v3_...): full reads, 7 planes
    "V3": [(-1, 4, 4, (1, 1, 0), _Z, _Z, 4, (1, 0, 7))],
    # rows per level: LEVEL_ROWS; entries per row of A on average: 7, 52, 443, 2719, 4567, 1115, 199
    "A1": [(-1, -1, -1, (1, 1, 0), (2, 1, 0), (1, 1, 0), 0, _Z),   # the 7-point fine operator: few column patterns - pattern-coded
           (-1, -1, -1, (2, 1, 0), (2, 1, 0), (2, 1, 0), 0, _Z),   # 52 per row: csr_stream_spmv
           (-1, -1, -1, (2, 1, 0), (2, 1, 0), (2, 1, 0), 0, _Z),   # 443 per row < longrow_min_avg
           (-1, -1, -1, (3, 1, 1), (2, 1, 0), (3, 1, 1), 0, _Z),   # 2719 per row: csr_longrow_spmv, 16-bit column offsets (spans < 65 536); P 618 per row
           (-1, -1, -1, (3, 1, 1), (2, 0, 0), (3, 0, 1), 0, _Z),   # 4567 per row; P (64 MB) and R below the NT size
           (-1, -1, -1, (3, 0, 1), (1, 0, 0), (3, 0, 1), 0, _Z),   # dense 1115 x 1115: long rows; the dense P has one pattern
           (-1, -1, -1, (1, 0, 0), (1, 0, 0), (1, 0, 0), 0, _Z)],  # dense 199 x 199 < longrow_min_avg: one pattern
    # entries per row of A on average: 7, 51, 525, 3496, 3287, 945, 373, 313, 312
    "A2": [(-1, -1, -1, (1, 0, 0), (2, 0, 0), (1, 0, 0), 0, _Z),
           (-1, -1, -1, (2, 0, 0), (2, 0, 0), (2, 0, 0), 0, _Z),
           (-1, -1, -1, (2, 1, 0), (2, 0, 0), (2, 0, 0), 0, _Z),   # 525 per row (224 MB: NT); R 757 per row, rows of up to 1722 entries
           (-1, -1, -1, (3, 1, 1), (3, 1, 1), (3, 1, 1), 0, _Z),   # 3496 per row; P 1073, R 3837: the long-row kernel for all three
           (-1, -1, -1, (3, 1, 1), (1, 0, 0), (3, 0, 1), 0, _Z),   # 3287 per row; P 942 per row < longrow_min_avg
           (-1, -1, -1, (1, 0, 0), (1, 0, 0), (1, 0, 0), 0, _Z),   # dense levels of < 1000 rows: one pattern each
           (-1, -1, -1, (1, 0, 0), (1, 0, 0), (1, 0, 0), 0, _Z),
           (-1, -1, -1, (1, 0, 0), (1, 0, 0), (1, 0, 0), 0, _Z),
           (-1, -1, -1, (1, 0, 0), (2, 0, 0), (1, 0, 0), 0, _Z)],
    "SY": [(-1, -1, -1, (2, 0, 0), (2, 0, 0), (2, 0, 0), 0, _Z),   # random columns: no patterns - csr_stream_spmv; A and R have empty rows and rows > one chunk
           (-1, -1, -1, (3, 1, 0), (2, 0, 0), (1, 0, 0), 0, _Z)],  # 1078 per row: csr_longrow_spmv; a row spans 70 000 columns: 32-bit columns
}
# the same with nrhs columns: operator_stream_kernel()[:2] of (A, P, R) per level - (4, NT) csr_stream_spmm<MODE, NT>, (5, 2)
# csr_rowclass_lane_spmm, (6, rows per lane) csr_rowclass_lane_spmm2<MODE, rows per lane> (even nrhs: two columns per lane; three rows
# per lane for a square operator).  Operators without row classes (every A of V1 and A1, the small levels below rowclass_min_rows)
# take csr_stream_spmm.
_S0, _S1 = ((4, 0),) * 3, ((4, 1),) * 3
EXPECTED_BLOCK = {
    ("C5", 3): [((5, 2),) * 3, ((5, 2),) * 3, ((5, 2), (5, 2), (4, 0)), _S0, _S0],
    ("C5", 16): [((6, 3), (6, 2), (6, 2)), ((6, 3), (6, 2), (6, 2)), ((6, 3), (6, 2), (4, 0)), _S0, _S0],
    ("V1", 3): [((4, 1), (5, 2), (5, 2)), ((4, 1), (5, 2), (5, 2)), ((4, 0), (5, 2), (4, 0)), _S0, _S0],
    ("V1", 16): [((4, 1), (6, 2), (6, 2)), ((4, 1), (6, 2), (6, 2)), ((4, 0), (6, 2), (4, 0)), _S0, _S0],
    ("A1", 3): [_S1, _S1, _S1, _S1, ((4, 1), (4, 0), (4, 0)), _S0, _S0],
    ("A1", 16): [_S1, _S1, _S1, _S1, ((4, 1), (4, 0), (4, 0)), _S0, _S0],
    ("SY", 3): [_S0, ((4, 1), (4, 0), (4, 0))],      # no row classes: csr_stream_spmm on empty rows (level 1's A, P, R) and long rows
    ("SY", 16): [_S0, ((4, 1), (4, 0), (4, 0))],
}


def _clean_env(mp):
    for k in list(os.environ):
        if k.startswith("MG_"):
            mp.delenv(k)
    assert not [k for k in os.environ if k.startswith("MG_")]


@pytest.fixture(autouse=True)
def _defaults(monkeypatch):
    _clean_env(monkeypatch)


def _divsiggrad(mg, cells, symmetrise):
    mesh = mg.getRegularMesh([0.0, 1.0] * 3, cells)
    sigma = np.exp(np.random.default_rng(11).standard_normal(int(np.prod(cells))))
    A = mg.getNodalDivSigGradMatrix(mesh, sigma)
    A = (A + 1e-3 * abs(A).sum(axis=0).max() * sp.identity(A.shape[0], format="csr")).tocsr()
    if symmetrise:
        A = ((A + A.T) * 0.5).tocsr()
    A.sort_indices()
    return A, mesh


def _synthetic(mg):
    """Three levels of general CSR, sized so that the default thresholds pick the kernels: level 1 (120 000 rows, short random
    rows) is streamed by csr_stream_spmv - 60 empty rows, rows of 700-1900 entries that straddle the 2048-entry LDS chunks, one
    row of 3000 entries (longer than a chunk); level 2 (70 000 rows of 1000-1151 entries, among them multiples of 64) has
    longrow_min_avg entries per row on average: csr_longrow_spmv, and one row spanning all 70 000 columns (> 65 535: no 16-bit
    column offsets for this operator).  P and R are random with empty rows; the third level only closes the hierarchy."""
    rng = np.random.default_rng(41)
    n, nc, n3 = 120_000, 70_000, 50

    def rows_of(lens, ncols):
        cols = [np.sort(rng.choice(ncols, int(k), replace=False)) if k else np.empty(0, dtype=np.int64) for k in lens]
        indptr = np.concatenate([[0], np.cumsum(lens)])
        M = sp.csr_matrix((rng.standard_normal(int(indptr[-1])), np.concatenate(cols), indptr), shape=(len(lens), ncols))
        M.sort_indices()
        return M

    lens = rng.integers(1, 13, n)
    lens[rng.choice(n, 60, replace=False)] = 0
    lens[1000:1006] = [700, 1900, 650, 1400, 900, 1024]
    lens[50_000] = 3000
    lens[n - 1] = 1300                                     # (the last row of the last row block)
    A1 = rows_of(lens, n)
    pool = [np.sort(rng.choice(4000, k, replace=False)) for k in (1000, 1024, 1088, 1100, 1151, 1152, 1033, 1077)]
    starts = rng.integers(0, nc - 4000, nc)
    cols = [pool[i % len(pool)] + starts[i] for i in range(nc)]
    cols[30_000] = np.unique(np.concatenate([[0, nc - 1], rng.choice(nc, 1022, replace=False)]))
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])])
    A2 = sp.csr_matrix((rng.standard_normal(int(indptr[-1])), np.concatenate(cols), indptr), shape=(nc, nc))
    A2.sort_indices()
    assert A2.nnz >= 1000 * nc and (np.diff(A2.indptr) % 64 == 0).any()
    lp = rng.integers(1, 7, n)
    lp[rng.choice(n, 500, replace=False)] = 0
    lr = rng.integers(4, 30, nc)
    lr[rng.choice(nc, 300, replace=False)] = 0
    lr[77] = 2500
    A3 = (sp.identity(n3) * 4.0 + 0.1 * sp.random(n3, n3, density=0.2, random_state=5)).tocsr()
    A3.sort_indices()
    p = mg.getMGparam(np.float64, np.int64, 3, 8, 1, 0.0, "Jac", 0.8, 1, 1, "V")
    p.As, p.Ps, p.Rs = [A1, A2, A3], [rows_of(lp, nc), rows_of(rng.integers(0, 4, nc), n3)], [rows_of(lr, n), rows_of(rng.integers(40, 90, n3), nc)]
    p.relaxPrecs = [rng.standard_normal(n), rng.standard_normal(nc)]
    p.LU = spla.splu(sp.csc_matrix(A3))
    p.nrhs = 1
    p.Meshes = []
    return p


@pytest.fixture(scope="class")
def hier(request, mg, built):
    """The hierarchy of the requesting class (TestV1 ... TestC5 at the end of the module): built once per class, on the host."""
    name = request.cls.name
    with pytest.MonkeyPatch.context() as mp:
        _clean_env(mp)          # (the handle reads its options from the environment when it is created; no MG_SETUP_GPU: host setup)
        if name in GMG:
            A, mesh = mg.poisson_shifted(GMG[name]) if name == "C5" else _divsiggrad(mg, GMG[name], name == "V2")
            levels = 6 if name != "V2" else 7
            p = mg.getMGparam(np.float64, np.int64, levels, 8, 2, 0.0, "Jac", 0.8, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
            mg.MGsetup(A, mesh, p)
            assert len(p.As) == levels
        elif name in SA:
            cells, weights, steps = SA[name]
            A, _ = mg.anisotropic_divsiggrad(cells, weights=weights)
            p = mg.getMGparam(np.float64, np.int64, 14, 8, steps, 0.0, "SPAI", 1.0, 1, 1, "V", "Julia", 0.4, 0.0)
            mg.SA_AMGsetup(A, p, True, 1)
        else:
            p = _synthetic(mg)
        h = mg.to_device(p)
        yield name, p, h
        mg.clear_(p)


def _observed(h, p):
    from multigrid_jl_amd import device as D
    got = []
    for l in range(1, len(p.As)):
        band = h.band_form(l)
        got.append(tuple(h.operator_kernel_variant(l, w) for w in (D.MG_OP_A, D.MG_OP_P, D.MG_OP_R))
                   + tuple(tuple(h.operator_stream_kernel(l, w)[:3]) for w in (D.MG_OP_A, D.MG_OP_P, D.MG_OP_R))
                   + (h.sweep_residual_form(l)[0], (band[0], band[2], band[3])))
    return got


def _which_kernel_serves_each_level(hier):
    from multigrid_jl_amd import device as D
    name, p, h = hier
    got = _observed(h, p)
    print(f"\nOBSERVED {name}: rows {[a.shape[0] for a in p.As]}\n" + "\n".join(f"    {row!r}," for row in got))
    assert h.operator_rowclasses(1, D.MG_OP_A)[0] == 0
    if name == "SY":      # what SY is there for, on the matrices themselves and as the device sees them
        for M, w in ((p.As[0], D.MG_OP_A), (p.Rs[0], D.MG_OP_R)):
            lens = np.diff(M.indptr)
            assert lens.max() > 2048 and (lens == 0).any() and h.operator_stream_kernel(1, w)[3] == lens.max()
        assert (np.diff(p.Ps[0].indptr) == 0).any()
        A2, r = p.As[1], 30_000
        assert A2.indices[A2.indptr[r + 1] - 1] - A2.indices[A2.indptr[r]] > 65535 and (np.diff(A2.indptr) % 64 == 0).sum() >= 3 * (A2.shape[0] // 8)
    assert got == EXPECTED.get(name), f"{name}: observed\n{got!r}"


def _sa_level_sizes_are_the_recorded_ones(hier):
    name, p, _ = hier
    assert ([a.shape[0] for a in p.As], [a.nnz for a in p.As]) == (LEVEL_ROWS[name], LEVEL_NNZ[name])


def _smooth(n, mesh=None):
    if mesh is not None:
        nodes = [int(v) + 1 for v in mesh.n]
        f = np.ones(1)
        for m in reversed(nodes):          # (x fastest: row = i + n1 (j + n2 k))
            f = np.multiply.outer(f, np.sin(np.pi * (np.arange(m) + 1.0) / (m + 1.0)) + 0.25 * np.cos(np.pi * np.arange(m) / m))
        return f.ravel()
    i = np.arange(n, dtype=np.float64)      # (no grid: smooth in the row index)
    return np.sin(np.pi * (i + 1.0) / (n + 1.0)) + 0.25 * np.cos(np.pi * i / n)


def _scaled_normal(rng, n):
    return rng.standard_normal(n) * np.exp2(rng.integers(-8, 9, n)).astype(np.float64)


def _mesh(p, l):
    return p.Meshes[l - 1] if getattr(p, "Meshes", None) and len(p.Meshes) >= l else None


def _inputs(family, rng, A, mesh):
    """(x, b) of a level: (a) standard normal times 2^k, k uniform in [-8, 8]; (b) x a low-frequency field, b = A x + 1e-6 noise."""
    n = A.shape[0]
    if family == "a":
        return _scaled_normal(rng, n), _scaled_normal(rng, n)
    x = _smooth(n, mesh)
    return x, A @ x + 1e-6 * rng.standard_normal(n)


def _check_level(h, tag, l, A, d, P, R, x, b, xc, rng):
    """Every product of level l: both fused kernels, A with three (alpha, beta), P with beta = 1, R with beta = 0 on NaN, the
    two-stage pass stage by stage where the level has one."""
    import torch
    from multigrid_jl_amd import device as D
    n = A.shape[0]
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
    xcg, y0 = Guarded(P.shape[1], xc, out=False), _scaled_normal(rng, n)
    out = Guarded(n)
    out.v.copy_(torch.from_numpy(y0))
    h.spmv_dev(l, D.MG_OP_P, 1.0, xcg.v, 1.0, out.v)
    check_spmv(f"{tag} P spmv (1, 1)", out.host(), 1.0, Product(P, xc), 1.0, y0)
    out = Guarded(R.shape[0])
    h.spmv_dev(l, D.MG_OP_R, 1.0, xg.v, 0.0, out.v)
    check_spmv(f"{tag} R spmv (1, 0)", out.host(), 1.0, Product(R, x))
    del out, xcg
    form = h.sweep_residual_form(l)[0]
    if form != 0:
        t, r, xn = Guarded(n), Guarded(n), (Guarded(n) if form != 5 else None)
        nrm = h.sweep_residual_dev(l, bg.v, xg.v, t.v, r.v, xn.v if xn else None, form != 5)
        th, rh = t.host(), r.host()
        check_sweep(f"{tag} pass t", th, x, d, b, pr)
        check_residual(f"{tag} pass r", rh, b, Product(A, th))
        if form != 5:
            check_xpdr(f"{tag} pass xn", xn.host(), th, d, rh)
            want = norm_ld(rh)
            assert abs(nrm - want) <= 1e-13 * want, (tag, nrm, want)
    for g in (xg, bg):
        g.host_guards()


def _level_products_row_by_row(hier, family):
    name, p, h = hier
    rng = np.random.default_rng(17 if family == "a" else 29)
    for l in range(1, len(p.As)):
        A, P, R = p.As[l - 1], p.Ps[l - 1], p.Rs[l - 1]
        x, b = _inputs(family, rng, A, _mesh(p, l))
        xc = _scaled_normal(rng, P.shape[1]) if family == "a" else _smooth(P.shape[1], _mesh(p, l + 1))
        _check_level(h, f"{name} level {l} ({family})", l, A, np.asarray(p.relaxPrecs[l - 1], dtype=np.float64), P, R, x, b, xc, rng)


def _solve_matches_c_oracle(mg, hier):
    _solve_check(mg, hier[1])


def _setup_gpu_comparison(mg, hier, monkeypatch):
    """The same hierarchy built again with MG_SETUP_GPU=1 (this test only: the largest Galerkin products of the setup on the GPU): its
    level sizes are REPORTED against the host-built ones, not asserted equal; both hierarchies must pass the solve check."""
    name, p, _ = hier
    cells, weights, steps = SA[name]
    monkeypatch.setenv("MG_SETUP_GPU", "1")
    A, _ = mg.anisotropic_divsiggrad(cells, weights=weights)
    q = mg.getMGparam(np.float64, np.int64, 14, 8, steps, 0.0, "SPAI", 1.0, 1, 1, "V", "Julia", 0.4, 0.0)
    mg.SA_AMGsetup(A, q, True, 1)
    try:
        rows, nnz = [a.shape[0] for a in q.As], [a.nnz for a in q.As]
        same = len(q.As) == len(p.As) and all((a != b).nnz == 0 for a, b in zip(q.As, p.As) if a.shape == b.shape)
        diff = max((abs(a - b).max() / abs(b).max() for a, b in zip(q.As, p.As) if a.shape == b.shape and a.nnz == b.nnz), default=None)
        print(f"\nSETUP_GPU {name}: level_rows equal {rows == LEVEL_ROWS[name]}, level_nnz equal {nnz == LEVEL_NNZ[name]}, "
              f"operators equal bit for bit {same}, largest relative difference of a level's entries {diff!r}; rows {rows}")
        _solve_check(mg, q)
    finally:
        mg.clear_(q)
    monkeypatch.delenv("MG_SETUP_GPU")
    _solve_check(mg, p)


def _solve_check(mg, p):
    A, steps = p.As[0], p.maxOuterIter
    b = mg.seeded_rhs(A)
    x = np.zeros_like(b)
    mg.solveMG(p, b, x)
    co = c_oracle.COracle(p, 1)
    xo = np.zeros_like(b)
    it, rv = co.solveMG(b, xo, 0.0, steps, c_oracle.max_threads())
    assert it == steps and len(p.resvec) == steps + 1 and np.abs(rv - p.resvec).max() / rv[0] < 1e-10
    assert np.abs(x - xo).max() <= 1e-10 * np.abs(xo).max()
    assert abs(np.linalg.norm(b - A @ x) - p.resvec[-1]) <= 1e-10 * p.resvec[0]


def _spai_vectors_against_long_double(hier):
    """relaxPrecs[l] = omega diag(A) / colsumsq(A) (omega = 1) of every level against the same in long double: a column of k
    entries costs k roundings for the squares and their sum, one for the quotient, one for omega - gamma_{k+2}."""
    name, p, _ = hier
    for l, (A, d) in enumerate(zip(p.As, p.relaxPrecs), 1):
        At = sp.csc_matrix(A)
        ip, va, n = At.indptr, At.data, A.shape[0]
        k = np.diff(ip)
        assert k.min() > 0
        diag = A.diagonal()
        d = np.asarray(d, dtype=np.float64)

        step = max(1, int(2_000_000 // max(1, k.max())))        # (long-double temporaries of at most 2 M entries)

        def ref_bound(r0, r1):
            ss = np.concatenate([np.add.reduceat(np.square(va[ip[c0]:ip[min(r1, c0 + step)]].astype(LD)), ip[c0:min(r1, c0 + step)] - ip[c0])
                                 for c0 in range(r0, r1, step)])
            ref = diag[r0:r1].astype(LD) / ss
            return ref, gamma(k[r0:r1] + 2) * np.abs(ref).astype(np.float64)

        C._check(f"{name} level {l} SPAI vector", d, ref_bound)


# ---- V3: one entry of the fine operator changed on the resident V2 hierarchy --------------------------------------------------------
def _with_fine_values(h, p, A, d):
    from multigrid_jl_amd import device as D
    h.replace_values(1, D.MG_OP_A, A)
    D._check(h.lib, h.lib.mg_set_relax_FP64(h.handle, 1, D._f64(d), d.size, int(p.relaxPre(1)), int(p.relaxPost(1))), "mg_set_relax")
    D._check(h.lib, h.lib.mg_finalize(h.handle), "mg_finalize")


def _perturbed(p, factor=None):
    """V2's fine operator with the stored +x entry a_ij (j = i + 1) of the grid's central node scaled by `factor` (None: moved by
    one ulp), and its Jacobi vector (the diagonal does not change)."""
    A = p.As[0].copy()
    n1, n2, n3 = (int(v) + 1 for v in p.Meshes[0].n)
    i = (n1 // 2) + n1 * ((n2 // 2) + n2 * (n3 // 2))
    s, e = A.indptr[i], A.indptr[i + 1]
    k = s + int(np.searchsorted(A.indices[s:e], i + 1))
    assert A.indices[k] == i + 1 and e - s == 7
    A.data[k] = A.data[k] * factor if factor is not None else np.nextafter(A.data[k], np.inf)
    assert A.data[k] != p.As[0].data[k] and A[i + 1, i] == p.As[0].data[k]
    return A, i, i + 1


def _v3_one_changed_entry_is_read_from_its_own_plane(hier):
    name, p, h = hier
    A0, d = p.As[0], np.asarray(p.relaxPrecs[0], dtype=np.float64)
    assert h.band_form(1) == [1, 1, 1, 4]                       # V2: symmetric bit for bit, 4 of 7 value planes
    A, i, j = _perturbed(p, 1.0 + 2.0 ** -20)
    rng = np.random.default_rng(53)
    x, b = _inputs("a", rng, A, p.Meshes[0])
    x[i] = np.copysign(max(abs(x[i]), 1.0), x[i])
    # teeth: symmetric reads would take a_ji from the new a_ij - row j moves by |a_ij - a_ji| |x_i|, at least 2^10 of its bounds
    pr = Product(A, x)
    delta = abs(A[i, j] - A[j, i]) * abs(x[i])
    assert delta >= 2.0 ** 10 * gamma(7 + 2) * (2.0 * abs(b[j]) + pr.abs[j])
    assert abs(d[j]) * delta >= 2.0 ** 10 * gamma(7 + 3) * (abs(x[j]) + abs(d[j]) * (abs(b[j]) + pr.abs[j]))
    try:
        _with_fine_values(h, p, A, d)
        assert h.band_form(1) == [1, 1, 0, 7] and _observed(h, p)[:1] == EXPECTED["V3"]     # full reads
        _check_level(h, "V3 level 1 (a)", 1, A, d, p.Ps[0], p.Rs[0], x, b, _scaled_normal(rng, p.Ps[0].shape[1]), rng)
        A1, _, _ = _perturbed(p, None)                           # (ii) one ulp: below any product check - the read path alone
        _with_fine_values(h, p, A1, d)
        assert h.band_form(1) == [1, 1, 0, 7]
    finally:
        _with_fine_values(h, p, A0, d)
    assert h.band_form(1) == [1, 1, 1, 4]


# ---- blocks of right-hand sides -----------------------------------------------------------------------------------------------
NAMED = (0, 1, 2, 7, 14, 15)
ZERO = 1            # the column of zeros: not the last one of an odd block (that remainder column carries a real product)


def _block_inputs(A, mesh, nrhs):
    """Family (b) for every column: the smooth field, shifted by 13 j rows so that no two columns are multiples of each other,
    times 2^(3j - 20); column ZERO is zero."""
    x = _smooth(A.shape[1], mesh)
    X = np.empty((A.shape[1], nrhs))
    for j in range(nrhs):
        X[:, j] = np.roll(x, 13 * j) * 2.0 ** (3 * j - 20)
    X[:, ZERO] = 0.0
    return X


def _block_out(out, cols):
    """The checked host copy of a block output; where only `cols` get a reference, no entry of any column may be NaN (outputs
    start NaN-filled: an unwritten or poisoned entry of the other columns shows here)."""
    G = out.host2d()
    if cols is not None:
        assert not np.isnan(G).any(), "an entry of a column without a reference is NaN"
    return G


def _block_products_column_by_column(hier, nrhs):
    import torch
    from multigrid_jl_amd import device as D
    name, p, h = hier
    L = len(p.As)

    def option(v):
        D._check(h.lib, h.lib.mg_set_option(h.handle, b"no_columns", v), "mg_set_option")
        D._check(h.lib, h.lib.mg_finalize(h.handle), "mg_finalize")

    rng = np.random.default_rng(61 + nrhs)
    try:
        h.set_nrhs(nrhs)
        option(1.0)
        got = [tuple(tuple(h.operator_stream_kernel(l, w)[:2]) for w in (D.MG_OP_A, D.MG_OP_P, D.MG_OP_R)) for l in range(1, L)]
        print(f"\nOBSERVED {name} nrhs {nrhs}:\n" + "\n".join(f"    {row!r}," for row in got))
        for l in range(1, L):
            A, P, R = p.As[l - 1], p.Ps[l - 1], p.Rs[l - 1]
            d = np.asarray(p.relaxPrecs[l - 1], dtype=np.float64)
            n, tag = A.shape[0], f"{name} level {l} nrhs {nrhs}"
            cols = NAMED if (l == 1 and nrhs == 16 and n > 4_000_000) else None
            X = _block_inputs(A, _mesh(p, l), nrhs)
            B = A @ X
            noise = 1e-6 * rng.standard_normal(n)
            for j in range(nrhs):
                B[:, j] += np.roll(noise, 5 * j) * 2.0 ** (3 * j - 20)
            xg, bg = Guarded.block(n, nrhs, X, out=False), Guarded.block(n, nrhs, B, out=False)
            prods = {}
            out = Guarded.block(n, nrhs)
            h.fused_dev(l, D.MG_K_RESIDUAL, bg.v, xg.v, out.v, nrhs)
            check_block(f"{tag} fused residual", "residual", _block_out(out, cols), A, X, cols, B=B, prods=prods)
            out = Guarded.block(n, nrhs)
            h.fused_dev(l, D.MG_K_SMOOTH, bg.v, xg.v, out.v, nrhs)
            check_block(f"{tag} fused smooth", "sweep", _block_out(out, cols), A, X, cols, B=B, d=d, prods=prods)
            for alpha, beta in ((0.5, -2.0), (1.0, 0.0)):
                out = Guarded.block(n, nrhs)
                if beta != 0.0:
                    out.v.copy_(torch.from_numpy(np.ascontiguousarray(B).ravel()))
                h.spmv_dev(l, D.MG_OP_A, alpha, xg.v, beta, out.v, nrhs)
                check_block(f"{tag} A spmm ({alpha}, {beta})", "spmv", _block_out(out, cols), A, X, cols, alpha=alpha, beta=beta, Y0=B, prods=prods)
            prods.clear()
            Xc = _block_inputs(P, _mesh(p, l + 1), nrhs)
            xcg = Guarded.block(P.shape[1], nrhs, Xc, out=False)
            out = Guarded.block(n, nrhs)
            out.v.copy_(torch.from_numpy(np.ascontiguousarray(B).ravel()))
            h.spmv_dev(l, D.MG_OP_P, 1.0, xcg.v, 1.0, out.v, nrhs)
            check_block(f"{tag} P spmm (1, 1)", "spmv", _block_out(out, cols), P, Xc, cols, alpha=1.0, beta=1.0, Y0=B)
            out = Guarded.block(R.shape[0], nrhs)
            h.spmv_dev(l, D.MG_OP_R, 1.0, xg.v, 0.0, out.v, nrhs)
            check_block(f"{tag} R spmm (1, 0)", "spmv", _block_out(out, cols), R, X, cols)
            for g in (xg, bg, xcg):
                g.host_guards()
            del out, xg, bg, xcg
        assert got == EXPECTED_BLOCK.get((name, nrhs)), f"{name} nrhs {nrhs}: observed\n{got!r}"
    finally:
        h.set_nrhs(1)
        option(0.0)


class _Single:
    def test_which_kernel_serves_each_level(self, hier):
        _which_kernel_serves_each_level(hier)

    @pytest.mark.parametrize("family", ["a", "b"])
    def test_level_products_row_by_row(self, hier, family):
        _level_products_row_by_row(hier, family)


class _Solved:
    def test_solve_matches_c_oracle(self, mg, hier):
        _solve_matches_c_oracle(mg, hier)


class _SaAmg:
    def test_sa_level_sizes_are_the_recorded_ones(self, hier):
        _sa_level_sizes_are_the_recorded_ones(hier)

    def test_spai_vectors_against_long_double(self, hier):
        _spai_vectors_against_long_double(hier)


class _Blocks:
    @pytest.mark.parametrize("nrhs", [3, 16])
    def test_block_products_column_by_column(self, hier, nrhs):
        _block_products_column_by_column(hier, nrhs)


class TestV1(_Single, _Solved, _Blocks):
    name = "V1"


class TestV2(_Single, _Solved):
    name = "V2"

    def test_v3_one_changed_entry_is_read_from_its_own_plane(self, hier):
        _v3_one_changed_entry_is_read_from_its_own_plane(hier)


class TestA1(_Single, _Solved, _SaAmg, _Blocks):
    name = "A1"


class TestA2(_Single, _Solved, _SaAmg):
    name = "A2"

    def test_setup_on_the_gpu_builds_a_hierarchy_that_solves(self, mg, hier, monkeypatch):
        _setup_gpu_comparison(mg, hier, monkeypatch)


class TestSY(_Single, _Blocks):
    name = "SY"


class TestC5(_Blocks):
    name = "C5"


assert all((n in SINGLE) == issubclass(c, _Single) and (n in SOLVED) == issubclass(c, _Solved) and (n in SA) == issubclass(c, _SaAmg)
           and (n in BLOCKS) == issubclass(c, _Blocks) for n, c in (("V1", TestV1), ("V2", TestV2), ("A1", TestA1), ("A2", TestA2), ("SY", TestSY), ("C5", TestC5)))


def test_each_kernel_serves_some_level():
    """Across the tables above (which the introspection tests hold to what the device reports): the band form with full reads
    and with symmetric reads, band-27, pattern-coded CSR, csr_stream_spmv and csr_longrow_spmv (each for some A; the long-row
    kernel with and without 16-bit column offsets), and the four block kernels."""
    rows = [row for t in EXPECTED.values() for row in t]
    assert any(row[6] == 4 and row[7] == (1, 0, 7) for row in rows), "band form, full reads"
    assert any(row[6] == 4 and row[7] == (1, 1, 4) for row in rows), "band form, symmetric reads"
    assert any(row[0] == 9 and row[7][0] == 2 for row in rows), "band-27"
    assert any(row[3][0] == 1 for row in rows), "csr_pattern_spmv"
    sa = [row for name in ("A1", "A2") for row in EXPECTED[name]]
    assert any(row[3][0] == 2 for row in sa), "csr_stream_spmv serves an A of A1 / A2"
    assert any(row[3][0] == 3 for row in sa), "csr_longrow_spmv serves an A of A1 / A2"
    assert any(row[3] == (3, row[3][1], 1) for row in rows) and any(row[3] == (3, row[3][1], 0) for row in rows)
    # a served operator with empty rows and one with a row longer than an LDS chunk (2048 entries): SY's A and R (SA's own
    # operators have neither an empty row nor, among those csr_stream_spmv serves, a row of more than 1722 entries)
    assert EXPECTED["SY"][0][3][0] == 2 and EXPECTED["SY"][0][5][0] == 2
    cells = [c for t in EXPECTED_BLOCK.values() for row in t for c in row]
    assert any(c[0] == 5 for c in cells), "csr_rowclass_lane_spmm"
    assert any(c[0] == 6 for c in cells), "csr_rowclass_lane_spmm2"
    assert any(c == (4, 1) for c in cells), "csr_stream_spmm<MODE, true>"
    assert any(c == (4, 0) for c in cells), "csr_stream_spmm<MODE, false>"
