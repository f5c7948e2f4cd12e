"""-m "not gpu": the host algebra of the Krylov drivers (csrc/mg_krylov_host.hpp) on its own, against numpy.

tests/native/krylov_host_algebra.cpp includes nothing but that header; it is built here with AddressSanitizer and
UndefinedBehaviorSanitizer and run as a child process on a file of cases.  A sanitizer report ends the program with a non-zero status and
text on stderr, and either fails the test.

Bounds.  Hessenberg least squares: the test draws Hbar until cond(Hbar) <= 100, so m * cond * eps <= 10 * 100 * 2.2e-16 ~ 2e-13 for both
the Givens route and numpy's SVD route; 1e-12 leaves a factor 5 to 10.  The estimate is compared relative to itself, y relative to ||y||.
The complex instantiation on real input runs the same operations except the radius (sqrt(|a|^2 + b^2) against hypot): 1e-14.
Relaxation: t goes through the normal equations, cond(H) <= 1e4 -> cond * eps ~ 2e-12, held to 1e-10; rn^2 = t'Ht - 2 t'xi + ||r0||^2 is
a sum of terms of size ||r0||^2, so 1e-12 ||r0||^2.  Dense helpers: 4 x 4, cond <= 100 -> 1e-12.
"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "krylov_host_algebra.cpp")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("krylov_host") / "krylov_host_algebra")
    # (the sanitizers' runtimes are linked statically: the program then runs whatever libraries the caller's environment loads ahead of it)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-o", exe, SRC], check=True, timeout=300)
    return exe


def _run(program, tmp_path, lines):
    """One child process over the cases in `lines` (lists of tokens); returns one array of floats per case."""
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(" ".join(repr(float(t)) if isinstance(t, (float, np.floating)) else str(t) for t in ln) for ln in lines) + "\n")
    p = subprocess.run([program, str(path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", f"exit {p.returncode}\n{p.stderr}"
    out = p.stdout.strip().split("\n")
    assert len(out) == len(lines) and all(o.split()[0] == ln[0] for o, ln in zip(out, lines))
    return [np.array([float(t) for t in o.split()[1:]]) for o in out]


def _flat(M):
    return [float(v) for v in np.asarray(M).ravel()]


def _hessenberg(rng, m, cx):
    """Hbar, (m + 1) x m upper Hessenberg with a real non-negative subdiagonal, cond <= 100."""
    for _ in range(10000):
        Hb = np.triu(rng.standard_normal((m + 1, m)) + (1j * rng.standard_normal((m + 1, m)) if cx else 0.0))
        Hb[np.arange(1, m + 1), np.arange(m)] = np.abs(rng.standard_normal(m))
        if np.linalg.cond(Hb) <= 100.0:
            return Hb
    raise AssertionError("no well-conditioned Hessenberg matrix drawn")


def _hess_case(Hb, beta, solve=1):
    m = Hb.shape[1]
    cx = np.iscomplexobj(Hb)
    toks = ["hess_cx" if cx else "hess_real", m, float(beta), solve]
    for i in range(m):
        for k in range(i + 1):
            toks += [float(Hb[k, i].real), float(Hb[k, i].imag)] if cx else [float(Hb[k, i])]
        toks.append(float(Hb[i + 1, i].real))
    return toks


def _hess_parse(out, m, cx):
    cols = out[:4 * m].reshape(m, 4)          # est, c_re, c_im, s
    y = out[4 * m:]
    return cols, (y[0::2] + 1j * y[1::2]) if cx else y


@pytest.mark.parametrize("cx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("m", [1, 2, 5, 10])
def test_hessenberg_lsq_against_lstsq(program, tmp_path, m, cx):
    rng = np.random.default_rng(1000 + 10 * m + cx)
    Hb = _hessenberg(rng, m, cx)
    assert np.linalg.cond(Hb) <= 100.0
    beta = float(np.abs(rng.standard_normal()) + 0.5)
    (out,) = _run(program, tmp_path, [_hess_case(Hb, beta)])
    cols, y = _hess_parse(out, m, cx)
    for i in range(m):
        rhs = np.zeros(i + 2, dtype=Hb.dtype)
        rhs[0] = beta
        yi = np.linalg.lstsq(Hb[:i + 2, :i + 1], rhs, rcond=None)[0]
        ref = np.linalg.norm(rhs - Hb[:i + 2, :i + 1] @ yi)
        print(f"m={m} column {i}: estimate {cols[i, 0]:.17g} lstsq {ref:.17g} rel {abs(cols[i, 0] - ref) / ref:.2e}")
        assert abs(cols[i, 0] - ref) <= 1e-12 * ref
    print(f"m={m}: y rel {np.linalg.norm(y - yi) / np.linalg.norm(yi):.2e}")
    assert np.linalg.norm(y - yi) <= 1e-12 * np.linalg.norm(yi)


@pytest.mark.parametrize("m", [1, 2, 5, 10])
def test_complex_instantiation_on_real_input_is_the_real_one(program, tmp_path, m):
    rng = np.random.default_rng(2000 + m)
    Hb = _hessenberg(rng, m, False)
    real, cplx = _run(program, tmp_path, [_hess_case(Hb, 1.25), _hess_case(Hb.astype(complex), 1.25)])
    (cr, yr), (cc, yc) = _hess_parse(real, m, False), _hess_parse(cplx, m, True)
    assert np.all(np.abs(cc[:, 0] - cr[:, 0]) <= 1e-14 * np.abs(cr[:, 0]))
    assert np.all(cc[:, 2] == 0.0) and np.all(yc.imag == 0.0)
    assert np.linalg.norm(cc[:, [1, 3]] - cr[:, [1, 3]]) <= 1e-14 * np.linalg.norm(cr[:, [1, 3]])
    assert np.linalg.norm(yc.real - yr) <= 1e-14 * np.linalg.norm(yr)


def test_degenerate_column_rotates_by_the_identity(program, tmp_path):
    Hz = np.zeros((2, 1))
    real, cplx = _run(program, tmp_path, [_hess_case(Hz, 2.0, solve=0), _hess_case(Hz.astype(complex), 2.0, solve=0)])
    for out in (real, cplx):
        assert np.all(np.isfinite(out))
        assert list(out) == [0.0, 1.0, 0.0, 0.0]          # |s_1| = 0, c = 1, s = 0


def _relax_case(AZ, r0):
    H = AZ.T @ AZ
    return ["relax", AZ.shape[1], float(np.linalg.norm(r0))] + _flat(H) + _flat(AZ.T @ r0)


@pytest.mark.parametrize("k", [1, 2, 4])
def test_relax_lsq_against_pinv(program, tmp_path, k):
    rng = np.random.default_rng(3000 + k)
    while True:
        AZ = rng.standard_normal((50, k))
        if np.linalg.cond(AZ.T @ AZ) <= 1e4:
            break
    assert np.linalg.cond(AZ.T @ AZ) <= 1e4
    r0 = rng.standard_normal(50)                             # (generic: not in the span of k <= 4 columns)
    (out,) = _run(program, tmp_path, [_relax_case(AZ, r0)])
    t, rn = out[:k], out[k]
    ref = np.linalg.pinv(AZ.T @ AZ) @ (AZ.T @ r0)
    print(f"k={k}: t rel {np.linalg.norm(t - ref) / np.linalg.norm(ref):.2e}  rn^2 abs/||r0||^2 "
          f"{abs(rn * rn - np.linalg.norm(r0 - AZ @ t) ** 2) / np.dot(r0, r0):.2e}")
    assert np.linalg.norm(t - ref) <= 1e-10 * np.linalg.norm(ref)
    assert abs(rn * rn - np.linalg.norm(r0 - AZ @ t) ** 2) <= 1e-12 * np.dot(r0, r0)


def test_relax_lsq_rank_deficient(program, tmp_path):
    rng = np.random.default_rng(3100)
    AZ = rng.standard_normal((50, 3))
    AZ[:, 2] = AZ[:, 0]                                       # a repeated direction: H is singular, t is not unique
    r0 = rng.standard_normal(50)
    (out,) = _run(program, tmp_path, [_relax_case(AZ, r0)])
    t, rn = out[:3], out[3]
    fit = AZ @ np.linalg.lstsq(AZ, r0, rcond=None)[0]
    assert np.linalg.norm(AZ @ t - fit) <= 1e-10 * np.linalg.norm(fit)
    assert abs(rn * rn - np.linalg.norm(r0 - fit) ** 2) <= 1e-12 * np.dot(r0, r0)


def _well_conditioned(rng, shape):
    while True:
        A = rng.standard_normal(shape)
        if np.linalg.cond(A) <= 100.0:
            return A


def test_small_dense_helpers(program, tmp_path):
    rng = np.random.default_rng(4000)
    A, B = _well_conditioned(rng, (4, 4)), rng.standard_normal((4, 2))
    Hs, Hr = _well_conditioned(rng, (4, 4)), _well_conditioned(rng, (6, 4))
    xs, xr = rng.standard_normal((4, 2)), rng.standard_normal((6, 2))
    while True:
        W = rng.standard_normal((10, 4))
        G = W.T @ W
        if np.linalg.cond(G) <= 100.0:
            break
    for M in (A, Hs, Hr, G):
        assert np.linalg.cond(M) <= 100.0
    solve, lsq_sq, lsq_rect, chol = _run(program, tmp_path, [
        ["solve", 4, 2] + _flat(A) + _flat(B), ["lstsq", 4, 4, 2] + _flat(Hs) + _flat(xs), ["lstsq", 6, 4, 2] + _flat(Hr) + _flat(xr),
        ["cholpinv", 4] + _flat(G)])

    def close(got, ref):
        return np.linalg.norm(np.asarray(got).ravel() - np.asarray(ref).ravel()) <= 1e-12 * np.linalg.norm(ref)

    assert close(solve, np.linalg.solve(A, B))
    assert close(lsq_sq[:8], np.linalg.solve(Hs, xs)) and lsq_sq[8] == 0.0          # (square: no rows left for a residual)
    Yr = np.linalg.lstsq(Hr, xr, rcond=None)[0]
    assert close(lsq_rect[:8], Yr) and close(lsq_rect[8], np.linalg.norm(xr - Hr @ Yr))
    Rref = np.linalg.cholesky(G).T
    assert close(chol[:16], Rref) and close(chol[16:], np.linalg.inv(Rref))


def test_krylov_report(program, tmp_path):
    vals = [0.5, 0.25, 0.125]
    (out,) = _run(program, tmp_path, [["report", len(vals)] + vals])
    assert list(out[:2]) == [0.0, 3.0]                                               # null pointers: accepted, records counted
    assert list(out[2:]) == [0.0, 5.0, -3.0, 3.0, 7.0, 0.25, 0.125, -1.0]          # MG_OK, iters, flag, nres, resvec (entry 0 set)
