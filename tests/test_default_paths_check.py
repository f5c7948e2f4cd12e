"""The row-by-row checker of tests/test_default_paths.py on the host: scipy's fp64 products pass its componentwise bounds,
a 1e-12 relative error in one small-magnitude row fails them (while a 1e-13 max-norm check on the whole vector passes it),
and a NaN in an output or a changed guard word fails."""
import numpy as np
import pytest
import scipy.sparse as sp

import default_paths_check as C


def _operator(mg):
    A, _ = mg.poisson_shifted([20, 17, 9])
    A = A.tolil()
    A[5, :] = 0.0          # (an empty row: the reference must give 0 there)
    A = A.tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    assert np.diff(A.indptr)[5] == 0
    return A


def _inputs(A, seed=3):
    rng = np.random.default_rng(seed)
    n = A.shape[0]
    x = rng.standard_normal(n) * np.exp2(rng.integers(-8, 9, n))
    b = rng.standard_normal(n) * np.exp2(rng.integers(-8, 9, n))
    d = 0.8 / np.where(A.diagonal() != 0, A.diagonal(), 1.0)
    return x, b, d


def test_fp64_products_pass(mg, monkeypatch):
    A = _operator(mg)
    monkeypatch.setattr(C, "CHUNK", 1000)        # (several pieces, several threads)
    x, b, d = _inputs(A)
    pr = C.Product(A, x)
    assert pr.ax[5] == 0 and pr.abs[5] == 0
    C.check_residual("residual", b - A @ x, b, pr)
    C.check_sweep("sweep", x + d * (b - A @ x), x, d, b, pr)
    C.check_spmv("spmv", -(A @ x) + b, -1.0, pr, 1.0, b)
    C.check_spmv("spmv", 0.5 * (A @ x) - 2.0 * b, 0.5, pr, -2.0, b)
    C.check_spmv("spmv beta 0", A @ x, 1.0, pr)
    P = sp.random(A.shape[0], 300, density=0.01, random_state=4, format="csr")
    xc = np.random.default_rng(5).standard_normal(300)
    C.check_spmv("transfer", P @ xc, 1.0, C.Product(P, xc))
    r = b - A @ x
    t = x + d * r
    C.check_xpdr("xpdr", t + d * r, t, d, r)
    assert abs(C.norm_ld(r) - np.linalg.norm(r)) <= 1e-14 * np.linalg.norm(r)


def test_small_row_error_fails_where_the_max_norm_check_passes(mg):
    A = _operator(mg)
    x, b, _ = _inputs(A)
    pr = C.Product(A, x)
    want = b - A @ x
    # a row of small magnitude against the vector's largest, without much cancellation inside the row
    scale = np.abs(b) + abs(A) @ np.abs(x)
    row = int(np.argmin(np.where(np.abs(want) >= 0.25 * scale, np.abs(want), np.inf)))
    assert np.abs(want[row]) <= 1e-3 * np.abs(want).max()
    got = want.copy()
    got[row] *= 1.0 + 1e-12
    assert got[row] != want[row]
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()     # the vector-wide check of the older tests lets it pass
    with pytest.raises(AssertionError, match=f"first row {row}:"):
        C.check_residual("residual", got, b, pr)


def test_nan_or_changed_guard_fails(mg):
    A = _operator(mg)
    x, b, _ = _inputs(A)
    pr = C.Product(A, x)
    got = b - A @ x
    got[17] = np.nan
    with pytest.raises(AssertionError, match="first row 17:"):
        C.check_residual("residual", got, b, pr)
    n = 100
    base = np.full(n + 2 * C.GUARD, np.nan)
    base.view(np.int64)[: C.GUARD] = C.SENTINEL
    base.view(np.int64)[-C.GUARD:] = C.SENTINEL
    assert C.host_checked(base.copy()).shape == (n,)
    for pos in (C.GUARD - 1, C.GUARD + n):                             # the word just before / just after the view
        bad = base.copy()
        bad[pos] = 0.0
        with pytest.raises(AssertionError, match="guard"):
            C.host_checked(bad)
    inp = np.full(n + 2 * C.GUARD, np.nan)
    inp[C.GUARD:C.GUARD + n] = 1.0
    assert C.host_checked(inp.copy(), out=False).shape == (n,)
    inp[C.GUARD + n] = 1.0
    with pytest.raises(AssertionError, match="guard"):
        C.host_checked(inp, out=False)


def test_block_checker_on_a_10k_row_matrix(monkeypatch):
    """check_block against scipy's fp64 block product on 10^4 rows: passes; a value written to the neighbouring column, a
    NaN in the zero column and a -1e-300 there fail; the long-double product agrees with scipy's to fp64 rounding."""
    monkeypatch.setattr(C, "CHUNK", 1500)
    rng = np.random.default_rng(8)
    n, nrhs = 10_000, 5
    A = (sp.random(n, n, density=8.0 / n, random_state=9, format="csr") + sp.identity(n, format="csr") * 4.0).tocsr()
    A.sort_indices()
    X = rng.standard_normal((n, nrhs)) * np.exp2(3.0 * np.arange(nrhs) - 20.0)      # (column j scaled by 2^(3j - 20))
    X[:, 3] = 0.0
    B, Y0 = rng.standard_normal((n, nrhs)), rng.standard_normal((n, nrhs))
    d = 0.8 / A.diagonal()
    AX = A @ X
    pr = C.Product(A, X[:, 1])
    assert np.abs(pr.ax.astype(np.float64) - AX[:, 1]).max() <= 1e-14 * np.abs(pr.abs).max()
    assert C.check_block("residual", "residual", B - AX, A, X, B=B) == n * nrhs
    C.check_block("sweep", "sweep", X + d[:, None] * (B - AX), A, X, B=B, d=d)
    C.check_block("spmv", "spmv", 0.5 * AX - 2.0 * Y0, A, X, alpha=0.5, beta=-2.0, Y0=Y0)
    C.check_block("spmv beta 0", "spmv", AX, A, X, cols=(0, 3, 4))
    swapped = (B - AX).copy()
    swapped[77, 1], swapped[77, 2] = swapped[77, 2], swapped[77, 1]
    with pytest.raises(AssertionError, match="column 1: 1 of 10000 rows .* first row 77:"):
        C.check_block("residual", "residual", swapped, A, X, B=B)
    C.check_block("residual", "residual", swapped, A, X, cols=(0, 3, 4), B=B)        # (only the named columns are looked at)
    for bad in (np.nan, -1e-300):
        got = AX.copy()
        got[5, 3] = bad
        with pytest.raises(AssertionError, match=r"column 3 \(x = 0\): row 5 "):
            C.check_block("spmv", "spmv", got, A, X)
    got = AX.copy()
    got[5, 3] = -0.0
    C.check_block("spmv", "spmv", got, A, X)


def test_guarded_block_layout_on_the_host():
    """Guarded.block stores entry (i, j) at i * nrhs + j: checked through the host-side reshape it uses (no device here)."""
    data = np.arange(12.0).reshape(4, 3)
    flat = np.ascontiguousarray(data).ravel()
    assert flat[2 * 3 + 1] == data[2, 1]
    base = np.concatenate([np.full(C.GUARD, np.nan), flat, np.full(C.GUARD, np.nan)])
    assert np.array_equal(C.host_checked(base, out=False).reshape(4, 3), data)
