"""Shared inputs and checkers of the Float32 / ComplexF32 hybrid-Kaczmarz tests (test infrastructure): the single operators, a
literal restatement of deps/src/parRelax.h:7-43 for spValType = float / float complex WITH THE ROUNDINGS OF THE COMPILED
BINARY, the call of the reference's applyHybridKaczmarz_FP32_INT64 / _CFP32_INT64 (oracle/_ref/parRelax.so, built by
oracle/Makefile where the reference tree is present) and its stored outputs,
tests/golden/reference_binaries/kaczmarz_single_outputs.npz.  Used by tests/test_kaczmarz_single_host.py,
tests/test_kaczmarz_single_gpu.py and by the generator of that file.

The roundings: parRelax.h:27 writes `inner -= conj(valA[gIdx])*x[...]`, and conj() is <complex.h>'s DOUBLE complex
function.  In the single builds that statement therefore widens valA and x to double, forms the product in double (every
float*float product is exact there; each part of a complex product is one rounded double sum of two exact products),
subtracts it from the widened inner in double and rounds inner back to single - after every term.  `inner *= invD[row-1]`
and `x[...] += inner*valA[gIdx]` are single arithmetic: C99's plain formula (a+bi)(c+di) = (ac-bd) + (ad+bc)i with every
product and sum rounded to float."""
import ctypes as C
import os

import numpy as np
import scipy.sparse as sp

from kaczmarz_complex_cases import helmholtz_unsym

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "parRelax.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_binaries", "kaczmarz_single_outputs.npz")

OMEGA = 0.8
TYPES = {"FP32": np.float32, "CFP32": np.complex64}
# name -> (cells, domains, nrhs, numit); awkward: crafted (see awkward_inputs), its two lists take the place of the domains
CASES = {
    "grid2d": ([24, 20], [3, 2], 3, 2),
    "grid3d": ([6, 6, 6], [2, 2, 2], 1, 3),
    "awkward": (None, None, 2, 3),
}
PAIRS = [(name, t) for name in CASES for t in TYPES]
F32 = np.float32


def cast_operator(A, tname):
    """The operator in the stored type: complex64, or for FP32 the real part cast to float32 (CSR, stored order kept)."""
    A = sp.csr_matrix(A)
    A = (A if tname == "CFP32" else A.real).astype(TYPES[tname]).tocsr()
    A.sort_indices()
    return A


def single_block(n, nrhs, seed, tname, scale=1.0):
    """A seeded n x nrhs column-major block of the type (1-D for nrhs = 1)."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, nrhs)) + 1j * rng.standard_normal((n, nrhs))
    v = np.asfortranarray(((v if tname == "CFP32" else v.real) * scale).astype(TYPES[tname]))
    return v[:, 0].copy() if nrhs == 1 else v


def awkward_inputs():
    """(A complex128 csr, Arr 40 x 2 uint32): n = 150, a 5 % random pattern plus a diagonal of 3; row 0 full (150 entries:
    two 64-entry chunks and a tail), row 1 with 70 leading entries (one chunk and a tail), row 2 with entries in columns
    5..134 (130: two chunks and a tail of 2), the diagonals of those three rows 9.  Two sub-domain lists of length 40: 35 and
    33 random rows, then rows 0, 1, 2, 0 appended to the first (a row twice inside one list) and rows 2, 0 to the second
    (again in another list); the remaining slots are zero padding."""
    n = 150
    rng = np.random.default_rng(2024)
    M = sp.random(n, n, density=0.05, random_state=rng, format="lil", dtype=np.float64)
    M = M.astype(np.complex128)
    for i, j in zip(*M.nonzero()):
        M[i, j] = rng.uniform(-1, 1) + 1j * rng.uniform(-1, 1)
    for i in range(n):
        M[i, i] = 3.0
    for j in range(n):
        M[0, j] = rng.uniform(-1, 1) + 1j * rng.uniform(-1, 1)
    for j in range(70):
        M[1, j] = rng.uniform(-1, 1) + 1j * rng.uniform(-1, 1)
    for j in range(5, 135):
        M[2, j] = rng.uniform(-1, 1) + 1j * rng.uniform(-1, 1)
    for i in range(3):
        M[i, i] = 9.0
    A = M.tocsr()
    A.sort_indices()
    Arr = np.zeros((40, 2), dtype=np.uint32, order="F")
    first = list(rng.choice(np.arange(3, n), 35, replace=False)) + [0, 1, 2, 0]
    second = list(rng.choice(np.arange(3, n), 33, replace=False)) + [2, 0]
    Arr[:len(first), 0] = np.asarray(first) + 1
    Arr[:len(second), 1] = np.asarray(second) + 1
    return A, Arr


_inputs = {}


def case_inputs(mg, name, tname):
    """(A, mesh or None, Arr, invD, b, x0) of a CASES entry in the type tname: the operator cast to single, Arr the
    sub-domains' row lists (DDService.jl:2-18, no overlap; awkward: crafted), invD the stated formula, b and a NON-ZERO start
    x0 seeded blocks (n, or n x nrhs column-major).  Computed once per (name, type); callers copy what they modify."""
    if (name, tname) not in _inputs:
        from oracle import mg_oracle as orc
        cells, domains, nrhs, _ = CASES[name]
        if name == "awkward":
            A64, Arr = awkward_inputs()
            mesh = None
        else:
            A64, mesh = helmholtz_unsym(mg, cells)
            Arr = orc.getIndicesOfCellsArray(cells, [0] * len(cells), domains)
        A = cast_operator(A64, tname)
        n = A.shape[0]
        b = single_block(n, nrhs, 11, tname, 1.0 / np.sqrt(n))
        x0 = single_block(n, nrhs, 12, tname, 0.5 / np.sqrt(n))
        for a in (A.data, Arr, b, x0):
            a.setflags(write=False)
        _inputs[(name, tname)] = (A, mesh, Arr, invdiag_single(A, OMEGA), b, x0)
    return _inputs[(name, tname)]


def invdiag_single(A, omega):
    """The single invDiag as setupHybridKaczmarz states it: conj(a) a = re*re + im*im with both products and their sum rounded
    to float32 (real: a*a rounded), a row's terms added in float32 in stored order, omega / sum in double, rounded to single
    once.  np.float32 scalars: every operation below is one float32 operation."""
    A = sp.csr_matrix(A)
    out = np.empty(A.shape[0], dtype=A.dtype)
    cx = np.iscomplexobj(A.data)
    for i in range(A.shape[0]):
        s = F32(0.0)
        for a in A.data[A.indptr[i]:A.indptr[i + 1]]:
            s = s + ((a.real * a.real + a.imag * a.imag) if cx else a * a)
            assert type(s) is F32
        out[i] = F32(float(omega) / float(s))
    return out


def restate_apply_single(A, Arr, x, b, invD, numit, first_statement_in_single=False):
    """parRelax.h:7-43 for spValType = float / float complex and ONE thread, statement by statement on valA = AT.nzval =
    conj(A.data), with the binary's roundings (module docstring): the first statement on Python floats (doubles) with inner
    rounded to np.float32 after every term, the other two on np.float32 scalars.  first_statement_in_single = True is the
    plausible-but-wrong variant that keeps the first statement in single too.  x (n, or n x nrhs column-major, of A's
    dtype) is updated in place and returned."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    cx = np.iscomplexobj(A.data)
    assert A.dtype in (np.float32, np.complex64) and x.dtype == A.dtype and np.asarray(b).dtype == A.dtype
    rowptr, colA = A.indptr.tolist(), A.indices.tolist()
    valA = np.conj(A.data)
    vr = [F32(v) for v in valA.real]
    vi = [F32(v) for v in valA.imag] if cx else None
    invD = np.asarray(invD)
    dr = [F32(v) for v in invD.real]
    di = [F32(v) for v in invD.imag] if cx else None
    X = x.reshape(n, -1, order="F")
    B = np.asarray(b).reshape(n, -1, order="F")
    nrhs = X.shape[1]
    xr = [[F32(v) for v in X[:, c].real] for c in range(nrhs)]
    xi = [[F32(v) for v in X[:, c].imag] for c in range(nrhs)] if cx else None
    for _ in range(int(numit)):
        for domain in range(Arr.shape[1]):
            for row in Arr[:, domain].tolist():
                if row == 0:
                    continue
                r = row - 1
                ks = range(rowptr[r], rowptr[r + 1])
                for c in range(nrhs):
                    XR = xr[c]
                    if not cx:
                        inner = F32(B[r, c])                                   # inner = b[offset + row-1]
                        for g in ks:                                           # inner -= conj(valA[gIdx])*x[...]
                            if first_statement_in_single:
                                inner = inner - vr[g] * XR[colA[g]]
                            else:
                                inner = F32(float(inner) - float(vr[g]) * float(XR[colA[g]]))
                        inner = inner * dr[r]                                  # inner *= invD[row-1]
                        for g in ks:                                           # x[...] += inner*valA[gIdx]
                            XR[colA[g]] = XR[colA[g]] + inner * vr[g]
                        assert type(inner) is F32
                        continue
                    XI = xi[c]
                    inr, ini = F32(B[r, c].real), F32(B[r, c].imag)
                    for g in ks:
                        k = colA[g]
                        if first_statement_in_single:
                            ar, ai = vr[g], -vi[g]
                            inr = inr - (ar * XR[k] - ai * XI[k])
                            ini = ini - (ar * XI[k] + ai * XR[k])
                        else:
                            ar, ai, cr, ci = float(vr[g]), -float(vi[g]), float(XR[k]), float(XI[k])
                            inr = F32(float(inr) - (ar * cr - ai * ci))
                            ini = F32(float(ini) - (ar * ci + ai * cr))
                    inr, ini = inr * dr[r] - ini * di[r], inr * di[r] + ini * dr[r]
                    for g in ks:
                        k = colA[g]
                        XR[k] = XR[k] + (inr * vr[g] - ini * vi[g])
                        XI[k] = XI[k] + (inr * vi[g] + ini * vr[g])
                    assert type(inr) is F32 and type(XR[k]) is F32
    for c in range(nrhs):
        X[:, c] = (np.asarray(xr[c]) + 1j * np.asarray(xi[c])) if cx else np.asarray(xr[c])
    return x


def ref_apply(A, Arr, x, b, invD, numit, numCores=1):
    """The reference's own applyHybridKaczmarz_FP32_INT64 / _CFP32_INT64 with the ccall of parRelax.jl:61-79: AT.colptr /
    AT.nzval / AT.rowval of AT = A' are A's CSR arrays (1-based) with the values conjugated."""
    A = sp.csr_matrix(A)
    cx = np.iscomplexobj(A.data)
    vt = np.complex64 if cx else np.float32
    assert A.dtype == vt
    lib = C.CDLL(REF)
    f = lib.applyHybridKaczmarz_CFP32_INT64 if cx else lib.applyHybridKaczmarz_FP32_INT64
    i64p, f32p, u32p = C.POINTER(C.c_longlong), C.POINTER(C.c_float), C.POINTER(C.c_uint)
    f.restype = None
    f.argtypes = [i64p, f32p, i64p, C.c_longlong, C.c_longlong, u32p, f32p, f32p, C.c_longlong, C.c_longlong, f32p,
                  C.c_longlong, C.c_longlong]
    cp = np.ascontiguousarray(A.indptr, dtype=np.int64) + 1
    rv = np.ascontiguousarray(A.indices, dtype=np.int64) + 1
    nz = np.ascontiguousarray(np.conj(A.data), dtype=vt)
    Arr = np.asfortranarray(Arr, dtype=np.uint32)
    invD = np.ascontiguousarray(invD, dtype=vt)
    b = np.asfortranarray(b, dtype=vt)
    assert x.dtype == vt and x.flags.f_contiguous and x.shape == b.shape
    nrhs = 1 if x.ndim == 1 else x.shape[1]
    f(cp.ctypes.data_as(i64p), nz.ctypes.data_as(f32p), rv.ctypes.data_as(i64p), Arr.shape[1], Arr.shape[0],
      Arr.ctypes.data_as(u32p), x.ctypes.data_as(f32p), b.ctypes.data_as(f32p), nrhs, A.shape[0], invD.ctypes.data_as(f32p),
      int(numit), int(numCores))
    return x


def run_reference_case(mg, name, tname):
    """The reference binary on a (case, type) pair with numCores = 1, from the case's non-zero x0."""
    A, _, Arr, invD, b, x0 = case_inputs(mg, name, tname)
    return ref_apply(A, Arr, x0.copy(order="F"), b, invD, CASES[name][3], 1)


_outputs = {}


def reference_output(mg, name, tname):
    """What the reference binary returns for a (case, type) pair (computed or loaded once, read-only).  Where
    oracle/_ref/parRelax.so is built it is run and must equal the copy stored in kaczmarz_single_outputs.npz bit for bit;
    elsewhere the stored copy is returned.  Re-record with
    tests/golden/reference_binaries/make_kaczmarz_single_outputs.py after changing CASES or their inputs."""
    key = f"{name}_{tname}"
    if key not in _outputs:
        stored = dict(np.load(GOLDEN)) if os.path.exists(GOLDEN) else {}
        if not os.path.exists(REF):
            assert key in stored, f"{key}: {REF} not built and no stored output in {GOLDEN}"
            out = stored[key]
        else:
            out = np.asarray(run_reference_case(mg, name, tname))
            assert key in stored and stored[key].shape == out.shape and stored[key].dtype == out.dtype, \
                f"{key}: no stored output of this shape and type (re-record it)"
            assert np.array_equal(out, stored[key]), f"{key}: stored output is stale (re-record it)"
        out.setflags(write=False)
        _outputs[key] = out
    return _outputs[key]
