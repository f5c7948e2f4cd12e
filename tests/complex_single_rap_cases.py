"""Shared by tests/test_complex_single_rap_host.py and tests/test_complex_single_rap_gpu.py: ComplexF32 params with
``singleDeviceSetup``, new matrices on an unchanged pattern, and the yardsticks of a re-setup in HBM (mg_rap_CF32).

Yardstick of the products.  The device reads As[l] (complex64) and Rs[l], Ps[l] (float32), widens each value, forms every entry of
Rs[l]*(As[l]*Ps[l]) in ComplexF64 and rounds each part once to single.  The comparand is therefore scipy's complex128 product of the
operators AS READ BACK, widened: per real and imaginary part |got - ref| <= 2^-24 |ref| (the one rounding to single, round to nearest)
+ 1e-13 max|ref entry| (the double sum's own error in any order: the bound tests/test_complex_rap_gpu.py puts on the ComplexF64
product).  The host's complex64 chain rounds after every product and is no comparand.  The pattern must be the host's exactly.
relaxPrecs: ``getRelaxPrec`` of the read-back complex64 As[l] (evaluated in double, converted once): |got - ref| <= 2^-23 |ref| in
modulus - the two parts' roundings on either side of a double evaluation good to 1e-13 - with non-finite entries (empty rows) in the
same places.  Imports no device code of the package."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

C64 = np.complex64
U32 = 2.0 ** -24


def single_param(mg, levels, relax="SPAI", omega=1.0, pre=2, post=1, cyc="V", maxIter=12, tol=1e-5, coarse="NoMUMPS", flag=True, **kw):
    return mg.getMGparam(np.complex128, np.int64, levels, 8, maxIter, tol, relax, omega, pre, post, cyc, coarse, 0.5, 0.0,
                         singlePrecision=True, **({"singleDeviceSetup": True} if flag else {}), **kw)


def new_matrix(A, seed):
    """tests/test_complex_rap_gpu.py::_new_matrix rounded to complex64: A's pattern with a seeded complex factor on every entry plus a
    heterogeneous complex diagonal (50-150 % of the largest diagonal entry) - non-symmetric, more diagonally dominant than A."""
    rng = np.random.default_rng(seed)
    A = sp.csr_matrix(A, dtype=np.complex128)
    A2 = A.copy()
    A2.data = A.data * ((1.0 + 0.3 * rng.random(A.nnz)) + 0.2j * rng.random(A.nnz))
    dmax = np.abs(A.diagonal()).max()
    A2 = (A2 + sp.diags(dmax * (0.5 + rng.random(A.shape[0])) * (1.0 + 0.25j))).tocsr()
    A2.sort_indices()
    assert np.array_equal(A2.indptr, A.indptr) and np.array_equal(A2.indices, A.indices)
    assert np.abs((A2 - A2.T).data).max() > 0.01 * dmax
    return A2.astype(C64)


def product_excess(got, R, A, P):
    """max over the entries and their two parts of |got - ref| / (2^-24 |ref| + 1e-13 max|ref entry|), ref = R*(A*P) in complex128 of the
    widened operators; asserts that ``got`` (CSR, complex64) holds ref's pattern."""
    assert got.dtype == C64 and A.dtype == C64 and R.dtype == np.float32 and P.dtype == np.float32
    W = lambda M, dt: sp.csr_matrix(M, dtype=dt)
    ref = (W(R, np.float64) @ (W(A, np.complex128) @ W(P, np.float64))).tocsr()
    ref.sort_indices()
    assert np.array_equal(ref.indptr, got.indptr) and np.array_equal(ref.indices, got.indices)
    if ref.nnz == 0:
        return 0.0
    big = max(np.abs(ref.data.real).max(), np.abs(ref.data.imag).max())
    g = got.data.astype(np.complex128)
    worst = 0.0
    for part in (np.real, np.imag):
        bound = U32 * np.abs(part(ref.data)) + 1e-13 * big
        worst = max(worst, float((np.abs(part(g) - part(ref.data)) / bound).max()))
    return worst


def relax_excess(mg, got, A, relaxType, omega):
    """max |got - ref| / (2^-23 |ref|) over the finite entries, ref = getRelaxPrec of the complex64 A; asserts dtype and that the
    non-finite entries sit in the same places.  Returns (excess, number of finite entries)."""
    assert got.dtype == C64 and A.dtype == C64
    with np.errstate(all="ignore"):
        ref = mg.getRelaxPrec(A, relaxType, omega)
    assert ref.dtype == C64
    ok = np.isfinite(ref)
    assert np.array_equal(ok, np.isfinite(got))
    r = ref[ok].astype(np.complex128)
    err = np.abs(got[ok].astype(np.complex128) - r)
    # (SPAI of an empty row whose column is not empty is an exact zero: then got must be zero too)
    return float((err / np.maximum(2.0 ** -23 * np.abs(r), 1e-300)).max()), int(ok.sum())


def assert_refreshed(mg, p, relaxType, omega, tag=""):
    """param.As[1:] and relaxPrecs of a refreshed pointwise param against the yardsticks, level by level."""
    for l in range(len(p.As) - 1):
        ep = product_excess(p.As[l + 1], p.Rs[l], p.As[l], p.Ps[l])
        er, _ = relax_excess(mg, p.relaxPrecs[l], p.As[l], relaxType, omega)
        print(f"  {tag}level {l + 1}: As[{l + 2}] {ep:.3f} of its bound, relaxPrec {er:.3f} of its bound, longest row {np.diff(p.As[l + 1].indptr).max()}")
        assert ep <= 1.0 and er <= 1.0


# ---- the awkward operator of tests/test_complex_rap_gpu.py in single ---------------------------------------------------------------
def awkward_pattern(n, seed):
    """Square CSR pattern with 40 empty rows, rows of 400-900 entries, one row of 3000; every row that is not empty holds its diagonal."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 12, n)
    lens[rng.choice(n, 40, replace=False)] = 0
    lens[100:104] = [700, 650, 900, 400]
    lens[2000] = 3000
    rows, cols = [], []
    for i, k in enumerate(lens):
        c = rng.choice(n, int(k), replace=False)
        if k and i not in c:
            c[0] = i
        c = np.sort(c)
        rows.append(np.full(len(c), i))
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    A = sp.csr_matrix((np.ones(len(rows), dtype=C64), (rows, cols)), shape=(n, n))
    A.sort_indices()
    return A


def values(M, seed, cplx):
    """M's pattern with seeded values: complex64, or float32."""
    rng = np.random.default_rng(seed)
    if cplx:
        v = (rng.standard_normal(M.nnz) + 1j * rng.standard_normal(M.nnz)).astype(C64)
    else:
        v = rng.standard_normal(M.nnz).astype(np.float32)
    return sp.csr_matrix((v, M.indices.copy(), M.indptr.copy()), shape=M.shape)


def manual_param(mg, A, P, R, Ac, d):
    """A two-level ComplexF32 param with ``singleDeviceSetup`` around arbitrary operators; the coarsest solve is a well-conditioned
    matrix of its own (a two-level cycle never applies As[2], it only solves with param.LU)."""
    nc = P.shape[1]
    p = single_param(mg, 2, "Jac", 0.8, 1, 1, "V", 4, 1e-6)
    p.As, p.Ps, p.Rs = [A, Ac], [P], [R]
    p.relaxPrecs = [d]
    S = (sp.identity(nc) * (4.0 + 1j) + 0.1 * sp.random(nc, nc, density=0.05, random_state=5)).tocsc().astype(np.complex128)
    p.LU = spla.splu(S)
    p.nrhs = 1
    return p
