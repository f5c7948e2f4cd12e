"""Shared inputs of the ComplexF64 tests (test infrastructure): complex operators, hierarchies and the complex splu in the
reference's parLU layout.  Used by tests/test_complex_host.py, tests/test_complex_gpu.py and the generator of
tests/golden/reference_binaries/complex_outputs.npz."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def helmholtz(mg, cells, kh=0.5, damping=0.5):
    """Shifted Laplacian -Lap - (1 - damping*i) k^2 on a nodal grid with k*h = kh (the Laplacian's own scaling: its interior
    diagonal is 2*dim/h^2 in its units).  Returns (A complex csr, mesh)."""
    mesh = mg.getRegularMesh([0.0, 1.0] * len(cells), list(cells))
    L = mg.getNodalLaplacianMatrix(mesh).tocsr()
    inv_h2 = L.diagonal().max() / (2 * len(cells))
    A = (L.astype(np.complex128) - (1.0 - damping * 1j) * kh * kh * inv_h2 * sp.identity(L.shape[0], format="csr")).tocsr()
    A.sort_indices()
    return A, mesh


def random_complex(n, density, seed, diag=4.0):
    """Unsymmetric complex sparse matrix with a dominant complex diagonal (csr, sorted)."""
    rng = np.random.default_rng(seed)
    E = sp.random(n, n, density=density, random_state=seed, format="csr")
    F = sp.random(n, n, density=density, random_state=seed + 1, format="csr")
    A = (E + 1j * F + sp.diags(diag + rng.standard_normal(n) + 1j * rng.standard_normal(n))).tocsr()
    A.sort_indices()
    return A


def complex_rhs(n, seed=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def lu_layout(lu):
    """A complex splu in parLU's layout (deps/src/parLU.cpp:120-190): CSR L (diagonal last) and U (diagonal first), 1-based
    Int64 arrays, p and q with A[p, q] = L U - the arrays mg_set_coarse_lu_CF64_INT64 takes."""
    L = sp.csr_matrix(lu.L)
    U = sp.csr_matrix(lu.U)
    L.sort_indices()
    U.sort_indices()
    a64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
    c128 = lambda a: np.ascontiguousarray(a, dtype=np.complex128)
    return dict(Lp=a64(L.indptr) + 1, Lc=a64(L.indices) + 1, Lv=c128(L.data), Up=a64(U.indptr) + 1, Uc=a64(U.indices) + 1,
                Uv=c128(U.data), p=a64(np.argsort(lu.perm_r)) + 1, q=a64(np.argsort(lu.perm_c)) + 1,
                nnz=max(L.nnz, U.nnz))


def lu_pin_system():
    """The system of the reference-binary pin: a 2-D Helmholtz-like complex operator with an unsymmetric perturbation."""
    n = 24
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))
    L2 = sp.kronsum(T, T).tocsc()
    A = (L2 - (0.3 - 0.15j) * sp.identity(L2.shape[0]) + 0.05j * sp.random(L2.shape[0], L2.shape[0], density=3.0 / L2.shape[0],
                                                                             random_state=3)).tocsc()
    lu = spla.splu(A, permc_spec="MMD_AT_PLUS_A")
    b = complex_rhs(A.shape[0], 11)
    return A, lu, b


def ref_lu_solve_complex(so_path, lu, b):
    """Call the reference's applyLUsolve_CFP64_INT64 (parLU.cpp:69-72) with the factors in parLU's layout; x = U \\ (L \\ b[p])
    scattered by q.  One factorisation, one right-hand side, doTranspose = 0."""
    import ctypes as C
    lib = C.CDLL(so_path)
    f = lib.applyLUsolve_CFP64_INT64
    i64p, f64p = C.POINTER(C.c_longlong), C.POINTER(C.c_double)
    f.restype = None
    f.argtypes = [i64p, f64p, i64p, i64p, f64p, i64p, i64p, i64p, i64p, i64p, f64p, f64p,
                  C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong]
    F = lu_layout(lu)
    n = lu.shape[0]
    nn = np.full(2, n, dtype=np.int64)
    nnz = np.full(2, F["nnz"], dtype=np.int64)
    x = np.zeros(n, dtype=np.complex128)
    bw = np.ascontiguousarray(b, dtype=np.complex128).copy()      # the reference uses b as workspace
    P = lambda a: a.ctypes.data_as(i64p)
    D = lambda a: a.ctypes.data_as(f64p)
    f(P(F["Lp"]), D(F["Lv"]), P(F["Lc"]), P(F["Up"]), D(F["Uv"]), P(F["Uc"]), P(F["p"]), P(F["q"]), P(nn), P(nnz), D(x), D(bw),
      1, 1, 1, 1, 0)
    return x
