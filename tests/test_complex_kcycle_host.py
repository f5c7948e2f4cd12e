"""-m "not gpu": the host side of the ComplexF64 Jac-GMRES smoother and K-cycle.

1. tests/complex_kcycle_oracle.py (the checker of the device path) on a real operator with a real right-hand side equals
   oracle/mg_oracle.py's Jac-GMRES / K cycle within 1e-13.  Both oracles are given THE SAME hierarchy: the complex param is the real
   one with its operators and relaxPrecs cast to complex128 and the real coarsest factors applied to real and imaginary parts
   (_complexified).  A complex param set up on its own differs from the real one in the last bit of relaxPrecs (numpy's complex
   division omega / (a + 0i) against the real one) and of the coarsest solve (complex against real splu), and the K-cycle
   amplifies that: its two directions are M r and M A M r with M A close to the identity, cond(H) is up to 1.4e5 on this
   problem, and t = pinv(H) xi carries any last-bit difference times cond(H) - 1.5e-13 to 5.8e-12 in the cycle with two separately
   set-up params, although neither oracle is wrong.  With the same hierarchy the complex oracle's sums are the real oracle's
   (its small dense algebra is written in real and imaginary parts, see FGMRES_relaxation there) and the cycles agree bit for bit.
2. The complex least squares of the relaxation (RelaxLsqC of csrc/mg_krylov_host.hpp) on its own.  tests/native/relax_lsq_complex.cpp
   includes nothing but that header; it is built here with AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process
   on a file of cases, exactly as tests/test_krylov_host_algebra.py runs its program.  A sanitizer report ends the program with a
   non-zero status and text on stderr, and either fails the test.

Bounds of 2, as tests/test_krylov_host_algebra.py derives them for the real RelaxLsq: t goes through the normal equations,
cond(H) <= 1e4 -> cond * eps ~ 2e-12, held to 1e-10; rn^2 = t'Ht - 2 Re t'xi + ||r0||^2 is a sum of terms of size ||r0||^2, so
1e-12 ||r0||^2.  Real input runs the real RelaxLsq's rotations on each diagonal block of the embedding: 1e-14.
"""
import copy
import os
import subprocess

import numpy as np
import pytest

import complex_kcycle_oracle as korc
from oracle import mg_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "relax_lsq_complex.cpp")
EPS = np.finfo(float).eps


class _RealFactors:
    """The real param's coarsest factors on a complex right-hand side: real and imaginary part solved separately."""

    def __init__(self, lu):
        self.lu = lu

    def solve(self, b):
        b = np.asarray(b)
        return self.lu.solve(np.ascontiguousarray(b.real)) + 1j * self.lu.solve(np.ascontiguousarray(b.imag))


def _complexified(pr):
    """The hierarchy of the real param `pr` as a complex one: the same operators, relaxPrecs and coarsest factors, value for value."""
    pc = copy.copy(pr)
    pc.As = [M.astype(np.complex128) for M in pr.As]
    pc.relaxPrecs = [np.asarray(d, dtype=np.complex128) for d in pr.relaxPrecs]
    pc.LU = _RealFactors(pr.LU)
    pc.device = None
    return pc


@pytest.mark.parametrize("relax,cyc,pre,post", [("Jac-GMRES", "V", 2, 2), ("Jac-GMRES", "K", 2, 1), ("Jac", "K", 2, 1),
                                                ("SPAI", "K", 1, 1), ("Jac-GMRES", "W", 3, 3)])
def test_oracle_on_real_operator_equals_real_oracle(mg, relax, cyc, pre, post):
    A, mesh = mg.poisson_shifted([8, 8, 8])
    pr = mg.getMGparam(np.float64, np.int64, 3, 8, 4, 1e-10, relax, 0.8, pre, post, cyc, "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(A, mesh, pr)
    pc = _complexified(pr)
    b = mg.seeded_rhs(A)
    xr = orc.recursiveCycle(pr, b, np.zeros_like(b), 1)
    trace = []
    xc = korc.recursiveCycle(pc, b.astype(np.complex128), np.zeros(b.size, dtype=np.complex128), 1, trace=trace)
    print(f"{relax} {cyc}({pre},{post}) first cycle: {np.abs(xc - xr).max() / np.abs(xr).max():.2e}")
    assert np.abs(xc - xr).max() <= 1e-13 * np.abs(xr).max()
    xr = orc.recursiveCycle(pr, b, xr, 1)                     # from the first iterate: the residual branch
    xc = korc.recursiveCycle(pc, b.astype(np.complex128), xc, 1, trace=trace)
    print(f"{relax} {cyc}({pre},{post}) second cycle: {np.abs(xc - xr).max() / np.abs(xr).max():.2e}")
    assert np.abs(xc - xr).max() <= 1e-13 * np.abs(xr).max()
    if relax == "Jac-GMRES" or cyc == "K":
        assert trace and all(rec[3] == len(rec[4]) and 1 <= rec[3] <= rec[2] for rec in trace)
    mg.clear_(pr)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("relax_lsq_complex") / "relax_lsq_complex")
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


def _pairs(z):
    return [float(v) for c in np.asarray(z).ravel() for v in (c.real, c.imag)]


def _cx_case(H, xi, rnorm0, m=None):
    k = H.shape[0]
    m = k if m is None else m
    return ["relax_cx", k, m, float(rnorm0)] + _pairs(H) + _pairs(xi[:m])


def _parse_cx(out, k):
    return out[0:2 * k:2] + 1j * out[1:2 * k:2], out[2 * k]


def _draw(rng, k, cx=True):
    while True:
        B = rng.standard_normal((50, k)) + (1j * rng.standard_normal((50, k)) if cx else 0.0)
        if np.linalg.cond(B.conj().T @ B) <= 1e4:
            return B


@pytest.mark.parametrize("k", range(1, 9))
def test_complex_relax_lsq_against_pinv(program, tmp_path, k):
    rng = np.random.default_rng(5000 + k)
    B = _draw(rng, k)
    H = B.conj().T @ B
    assert np.linalg.cond(H) <= 1e4
    r0 = rng.standard_normal(50) + 1j * rng.standard_normal(50)
    xi = B.conj().T @ r0
    (out,) = _run(program, tmp_path, [_cx_case(H, xi, np.linalg.norm(r0))])
    t, rn = _parse_cx(out, k)
    Hs = 0.5 * (H + H.conj().T)
    ref = np.linalg.pinv(Hs, rcond=EPS * k) @ xi
    r2 = np.vdot(r0, r0).real
    print(f"k={k}: t rel {np.linalg.norm(t - ref) / np.linalg.norm(ref):.2e}  rn^2 abs/||r0||^2 "
          f"{abs(rn * rn - np.linalg.norm(r0 - B @ t) ** 2) / r2:.2e}")
    assert np.linalg.norm(t - ref) <= 1e-10 * np.linalg.norm(ref)
    assert abs(rn * rn - np.linalg.norm(r0 - B @ t) ** 2) <= 1e-12 * r2


@pytest.mark.parametrize("k,m", [(3, 1), (5, 2), (8, 3), (8, 7)])
def test_leading_block_equals_the_zero_padded_solve(program, tmp_path, k, m):
    """step(m) on a capacity of k: the reference's pinv of its zero-padded k x k H (cut-off eps * k * sigma_max), zeros behind m."""
    rng = np.random.default_rng(5100 + 10 * k + m)
    B = _draw(rng, k)
    H = B.conj().T @ B
    r0 = rng.standard_normal(50) + 1j * rng.standard_normal(50)
    xi = B.conj().T @ r0
    (out,) = _run(program, tmp_path, [_cx_case(H, xi, np.linalg.norm(r0), m)])
    t, rn = _parse_cx(out, k)
    Hp = np.zeros_like(H)
    Hp[:m, :m] = 0.5 * (H[:m, :m] + H[:m, :m].conj().T)
    xp = np.zeros_like(xi)
    xp[:m] = xi[:m]
    ref = np.linalg.pinv(Hp, rcond=EPS * k) @ xp
    assert np.all(t[m:] == 0.0)
    assert np.linalg.norm(t - ref) <= 1e-10 * np.linalg.norm(ref)
    assert abs(rn * rn - np.linalg.norm(r0 - B @ t) ** 2) <= 1e-12 * np.vdot(r0, r0).real


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_real_input_gives_the_real_relax_lsq(program, tmp_path, k):
    rng = np.random.default_rng(5200 + k)
    B = _draw(rng, k, cx=False)
    H = B.T @ B
    r0 = rng.standard_normal(50)
    xi = B.T @ r0
    real_case = ["relax_real", k, float(np.linalg.norm(r0))] + [float(v) for v in H.ravel()] + [float(v) for v in xi]
    cplx, real = _run(program, tmp_path, [_cx_case(H.astype(complex), xi.astype(complex), np.linalg.norm(r0)), real_case])
    t, rn = _parse_cx(cplx, k)
    tr, rnr = real[:k], real[k]
    assert np.all(t.imag == 0.0)
    assert np.linalg.norm(t.real - tr) <= 1e-14 * np.linalg.norm(tr)
    assert abs(rn - rnr) <= 1e-14 * np.linalg.norm(r0)


def test_rank_deficient_gives_numpys_pinv(program, tmp_path):
    rng = np.random.default_rng(5300)
    B = rng.standard_normal((50, 3)) + 1j * rng.standard_normal((50, 3))
    B[:, 2] = B[:, 0]                                        # a repeated direction: H is singular
    H = B.conj().T @ B
    r0 = rng.standard_normal(50) + 1j * rng.standard_normal(50)
    xi = B.conj().T @ r0
    (out,) = _run(program, tmp_path, [_cx_case(H, xi, np.linalg.norm(r0))])
    t, rn = _parse_cx(out, 3)
    ref = np.linalg.pinv(0.5 * (H + H.conj().T), rcond=EPS * 3) @ xi     # the minimum-norm solution: t[0] == t[2]
    assert np.linalg.norm(t - ref) <= 1e-10 * np.linalg.norm(ref)
    fit = B @ np.linalg.lstsq(B, r0, rcond=None)[0]
    assert abs(rn * rn - np.linalg.norm(r0 - fit) ** 2) <= 1e-12 * np.vdot(r0, r0).real
