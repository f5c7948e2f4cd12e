"""Shared inputs and bounds of the device-inverse tests (test infrastructure): tests/test_coarse_device_inverse_host.py and
tests/test_coarse_device_inverse_gpu.py.

The bound of an inverse.  res(X) = max(||A X - I||_F, ||X A - I||_F) / sqrt(n); the device result must meet
res(X_dev) <= 8 * max(res(numpy.linalg.inv(A)), n * eps).  The comparand is LAPACK's dense inverse with partial pivoting, the same
class of algorithm; the factor 8 covers another summation order, FMA contraction and blocking; the floor n * eps is there because
numpy's residual is exactly 0 on some tiny cases (the real 2 x 2 matrix below).  An unblocked numpy model of the device algorithm
(in-place Gauss-Jordan with the pivot rule max |re| + |im|, lowest row on ties) gives 0.35 - 0.9 times numpy's residual on the
matrices below (condition numbers 1 to 2.0e3).

The bound of cycles and solves: a param with ``coarseDeviceInverse=True`` against the same param without it - the same kernels on an
inverse that differs in its last bits: 1e-11 of max|x| for ComplexF64 and Float64, 64 * 2^-24 for ``singlePrecision``, the bounds of
tests/test_vanka_device_setup_gpu.py for "same kernels, only the origin of the data differs"."""
import numpy as np
import scipy.sparse as sp

EPS = np.finfo(np.float64).eps
COND_MAX = 1e4
TOL = {False: 1e-11, True: 64 * 2.0 ** -24}

# The orders the issue names, then the edges of the kernel: its panel width and its update tile are both 64, so 63 / 64 / 65 are one
# order below, at and above them (65 is named already) and 129 is two panels plus one column; 16 and 17 are the rows of one
# workgroup of the strip kernels and one more.
SIZES = [1, 2, 7, 31, 32, 33, 65, 200, 257, 16, 17, 63, 64, 129]


def matrix(n, cx):
    """standard_normal entries from default_rng(1000 + n) (plus i * standard_normal for complex), the diagonal zeroed for n > 1 so
    that nearly every column interchanges rows."""
    g = np.random.default_rng(1000 + n)
    A = g.standard_normal((n, n))
    if cx:
        A = A + 1j * g.standard_normal((n, n))
    if n > 1:
        np.fill_diagonal(A, 0.0)
    return np.asfortranarray(A)


def res(A, X):
    n = A.shape[0]
    I = np.eye(n)
    return max(np.linalg.norm(A @ X - I), np.linalg.norm(X @ A - I)) / np.sqrt(n)


def inverse_ratio(A, X):
    """res(X) over its bound's comparand max(res(numpy.linalg.inv(A)), n * eps): the test asserts <= 8."""
    A = np.asarray(A)
    return res(A, X) / max(res(A, np.linalg.inv(A)), A.shape[0] * EPS)


def exact_case(n, cx, seed=7):
    """A = P D with P a permutation and D a diagonal of signed powers of two (complex: every third entry purely imaginary):
    every pivot is the only non-zero of its column and nothing rounds.  Returns (A, inv(A) = D^-1 P' exactly)."""
    g = np.random.default_rng(seed + n)
    perm = g.permutation(n)
    d = (2.0 ** g.integers(-20, 21, n)) * g.choice([-1.0, 1.0], n)
    d = d.astype(np.complex128 if cx else np.float64)
    if cx:
        d[::3] *= 1j
    A = np.zeros((n, n), dtype=d.dtype)
    A[perm, np.arange(n)] = d              # A[:, j] = d_j e_perm[j]
    X = np.zeros((n, n), dtype=d.dtype)
    X[np.arange(n), perm] = 1.0 / d        # (1 / (i 2^e) = -i 2^-e: exact)
    return np.asfortranarray(A), np.asfortranarray(X)


def singular_cases(cx=False):
    """70 x 70: column 40 zeroed (it falls in the second panel), and a NaN entry."""
    A = matrix(70, cx)
    Z = A.copy(order="F")
    Z[:, 40] = 0.0
    N = A.copy(order="F")
    N[50, 10] = np.nan
    return Z, N


# ---- hierarchies: name -> (cells, levels, value type); the coarsest orders are 25, 125, 729 and 125 ---------------------------------
HCASES = {"8x8": ([8, 8], 2, "complex"), "8x8x8": ([8, 8, 8], 2, "complex"), "16x16x16": ([16, 16, 16], 2, "complex"),
          "real8x8x8": ([8, 8, 8], 2, "real")}


def operator(mg, name, damping=0.5, shift=1.0):
    """(A, mesh) of a case: complex_cases.helmholtz with ``damping``, or for the Float64 case the nodal Laplacian plus ``shift``
    times the identity."""
    import complex_cases as CC
    cells, levels, kind = HCASES[name]
    if kind == "complex":
        return CC.helmholtz(mg, cells, damping=damping)
    mesh = mg.getRegularMesh([0.0, 1.0] * len(cells), list(cells))
    L = mg.getNodalLaplacianMatrix(mesh).tocsr()
    A = (L + shift * sp.identity(L.shape[0], format="csr")).tocsr()
    A.sort_indices()
    return A, mesh


def param(mg, name, relaxType="Jac", single=False, flag=False, maxIter=4, **kw):
    cells, levels, kind = HCASES[name]
    val = np.complex128 if kind == "complex" else np.float64
    extra = dict(kw)
    if single:
        extra["singlePrecision"] = True
    if flag:
        extra["coarseDeviceInverse"] = True
    return mg.getMGparam(val, np.int64, levels, 1, maxIter, 1e-30, relaxType, 0.8, 2, 1, "V", "NoMUMPS", 0.4, 0.0, **extra)


def rhs(n, cx, single=False, seed=5):
    g = np.random.default_rng(seed)
    b = g.standard_normal(n) + (1j * g.standard_normal(n) if cx else 0.0)
    return b.astype(np.complex64) if single else b


def err_max(a, ref):
    return float(np.abs(np.asarray(a, dtype=np.complex128) - np.asarray(ref, dtype=np.complex128)).max() / np.abs(ref).max())
