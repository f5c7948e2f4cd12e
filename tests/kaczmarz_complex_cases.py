"""Shared inputs and checkers of the ComplexF64 hybrid-Kaczmarz tests (test infrastructure): the complex operators, a literal
restatement of deps/src/parRelax.h:7-43 for spValType = double complex, the call of the reference's compiled
applyHybridKaczmarz_CFP64_INT64 (oracle/_ref/parRelax.so, built by oracle/Makefile where the reference tree is present) and
its stored outputs, tests/golden/reference_binaries/kaczmarz_complex_outputs.npz.  Used by tests/test_kaczmarz_complex.py
and by the generator of that file."""
import ctypes as C
import os

import numpy as np
import scipy.sparse as sp

from complex_cases import helmholtz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "parRelax.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_binaries", "kaczmarz_complex_outputs.npz")

OMEGA = 0.8
# name -> (cells, domains, nrhs, numit)
CASES = {
    "kaczmarz_c_64x64_d4x4_nrhs2_it5": ([64, 64], [4, 4], 2, 5),
    "kaczmarz_c_10x10x10_d2x2x2_nrhs1_it3": ([10, 10, 10], [2, 2, 2], 1, 3),
    "kaczmarz_c_30x20_d3x2_nrhs3_it2": ([30, 20], [3, 2], 3, 2),
}


def helmholtz_unsym(mg, cells, seed=7, kh=0.5):
    """The shifted Laplacian of complex_cases.helmholtz plus an imaginary part on its strict upper triangle: complex,
    unsymmetric and non-Hermitian off the diagonal, so a missing or misplaced conj changes the sweep.  (A csr, mesh)."""
    A, mesh = helmholtz(mg, cells, kh=kh)
    U = sp.triu(A, 1, format="csr")
    rng = np.random.default_rng(seed)
    U.data = rng.uniform(-1.0, 1.0, U.nnz) * 0.1 * np.abs(A.diagonal()).max()
    A = (A + 1j * U).tocsr()
    A.sort_indices()
    return A, mesh


def complex_block(A, nrhs, seed):
    """A normalised complex right-hand side in A's range: 1-D for nrhs = 1, else n x nrhs column-major."""
    rng = np.random.default_rng(seed)
    b = A @ (rng.standard_normal((A.shape[0], nrhs)) + 1j * rng.standard_normal((A.shape[0], nrhs)))
    b = np.asfortranarray(b / np.linalg.norm(b))
    return b[:, 0].copy() if nrhs == 1 else b


def case_inputs(mg, name):
    """(A, mesh, Arr, invD, b) of a CASES entry; Arr is the sub-domains' row lists of DDService.jl:2-18 (no overlap)."""
    from oracle import mg_oracle as orc
    cells, domains, nrhs, _ = CASES[name]
    A, mesh = helmholtz_unsym(mg, cells)
    Arr = orc.getIndicesOfCellsArray(cells, [0] * len(cells), domains)
    return A, mesh, Arr, invdiag(A, OMEGA), complex_block(A, nrhs, 11)


def invdiag(A, omega):
    """parRelax.jl:33: convert(Array{ComplexF64,1}, omega ./ sum(conj(AT).*AT, dims=1)), as omega / s_i: column i of AT is
    row i of A, whose terms conj(a) a (C99 formula, Python floats) are summed in stored order."""
    A = sp.csr_matrix(A)
    out = np.empty(A.shape[0], dtype=np.complex128)
    for i in range(A.shape[0]):
        sr, si = 0.0, 0.0
        for a in A.data[A.indptr[i]:A.indptr[i + 1]].tolist():
            ar, ai = a.real, -a.imag                  # conj(a) * a
            sr, si = sr + (ar * a.real - ai * a.imag), si + (ar * a.imag + ai * a.real)
        assert si == 0.0
        out[i] = complex(omega / sr, 0.0)
    return out


def restate_apply(A, Arr, x, b, invD, numit):
    """parRelax.h:7-43 with spValType = double complex and ONE thread (sub-domains in order, rows of a sub-domain in order),
    statement by statement, on valA = AT.nzval = conj(A.data).  Every complex product is C99's plain formula
    (a+bi)(c+di) = (ac-bd) + (ad+bc)i in Python floats (each operation rounded once); `-=` / `+=` act on the real and imaginary
    parts separately.  x (n, or n x nrhs column-major, complex128) is updated in place and returned."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    rowptr, colA = A.indptr.tolist(), A.indices.tolist()
    valA = np.conj(A.data)
    vr, vi = valA.real.tolist(), valA.imag.tolist()
    dr, di = np.real(invD).tolist(), np.imag(invD).tolist()
    X = x.reshape(n, -1, order="F")
    B = np.asarray(b).reshape(n, -1, order="F")
    nrhs = X.shape[1]
    xr = [X[:, c].real.tolist() for c in range(nrhs)]
    xi = [X[:, c].imag.tolist() for c in range(nrhs)]
    br = [B[:, c].real.tolist() for c in range(nrhs)]
    bi = [B[:, c].imag.tolist() for c in range(nrhs)]
    for _ in range(int(numit)):
        for domain in range(Arr.shape[1]):
            for row in Arr[:, domain].tolist():
                if row > 0:
                    r = row - 1
                    for c in range(nrhs):
                        XR, XI = xr[c], xi[c]
                        inr, ini = br[c][r], bi[c][r]                    # inner = b[offset + row-1]
                        for g in range(rowptr[r], rowptr[r + 1]):        # inner -= conj(valA[gIdx])*x[...]
                            ar, ai = vr[g], -vi[g]
                            cr, ci = XR[colA[g]], XI[colA[g]]
                            inr = inr - (ar * cr - ai * ci)
                            ini = ini - (ar * ci + ai * cr)
                        inr, ini = inr * dr[r] - ini * di[r], inr * di[r] + ini * dr[r]   # inner *= invD[row-1]
                        for g in range(rowptr[r], rowptr[r + 1]):        # x[...] += inner*valA[gIdx]
                            k = colA[g]
                            XR[k] = XR[k] + (inr * vr[g] - ini * vi[g])
                            XI[k] = XI[k] + (inr * vi[g] + ini * vr[g])
    for c in range(nrhs):
        X[:, c] = np.asarray(xr[c]) + 1j * np.asarray(xi[c])
    return x


def ref_apply(A, Arr, x, b, invD, numit, numCores=1):
    """The reference's own applyHybridKaczmarz_CFP64_INT64 with the ccall of parRelax.jl:71-74: AT.colptr / AT.nzval /
    AT.rowval of AT = A' are A's CSR arrays (1-based) with the values conjugated."""
    lib = C.CDLL(REF)
    f = lib.applyHybridKaczmarz_CFP64_INT64
    i64p, f64p, u32p = C.POINTER(C.c_longlong), C.POINTER(C.c_double), C.POINTER(C.c_uint)
    f.restype = None
    f.argtypes = [i64p, f64p, i64p, C.c_longlong, C.c_longlong, u32p, f64p, f64p, C.c_longlong, C.c_longlong, f64p,
                  C.c_longlong, C.c_longlong]
    A = sp.csr_matrix(A)
    cp = np.ascontiguousarray(A.indptr, dtype=np.int64) + 1
    rv = np.ascontiguousarray(A.indices, dtype=np.int64) + 1
    nz = np.ascontiguousarray(np.conj(A.data), dtype=np.complex128)
    Arr = np.asfortranarray(Arr, dtype=np.uint32)
    invD = np.ascontiguousarray(invD, dtype=np.complex128)
    b = np.asfortranarray(b, dtype=np.complex128)
    assert x.dtype == np.complex128 and x.flags.f_contiguous and x.shape == b.shape
    nrhs = 1 if x.ndim == 1 else x.shape[1]
    f(cp.ctypes.data_as(i64p), nz.ctypes.data_as(f64p), rv.ctypes.data_as(i64p), Arr.shape[1], Arr.shape[0],
      Arr.ctypes.data_as(u32p), x.ctypes.data_as(f64p), b.ctypes.data_as(f64p), nrhs, A.shape[0], invD.ctypes.data_as(f64p),
      int(numit), int(numCores))
    return x


def reference_output(name, call):
    """What the reference binary returns for a CASES entry.  Where oracle/_ref/parRelax.so is built, call() runs it and must
    match the copy stored in kaczmarz_complex_outputs.npz; elsewhere the stored copy is returned.  Re-record with
    tests/golden/reference_binaries/make_kaczmarz_complex_outputs.py after changing CASES or their inputs."""
    stored = dict(np.load(GOLDEN)) if os.path.exists(GOLDEN) else {}
    if not os.path.exists(REF):
        assert name in stored, f"{name}: {REF} not built and no stored output in {GOLDEN}"
        return stored[name]
    out = np.asarray(call())
    assert name in stored and stored[name].shape == out.shape, f"{name}: no stored output of this shape (re-record it)"
    assert np.abs(out - stored[name]).max() <= 1e-12 * np.abs(out).max(), f"{name}: stored output is stale (re-record it)"
    return out


def run_reference_case(mg, name):
    """The reference binary on a CASES entry with numCores = 1, from x = 0."""
    A, _, Arr, invD, b = case_inputs(mg, name)
    numit = CASES[name][3]
    return ref_apply(A, Arr, np.zeros_like(b, order="F"), b, invD, numit, 1)
