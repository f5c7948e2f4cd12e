"""Blocks of right-hand sides on complex hierarchies, host side (no GPU): the block oracle (tests/complex_block_oracle.py) pinned to
the real block oracle and to the single-vector complex one, the counts the GPU tests rely on, the exported symbols, the Python
surface and its routing, and the k x k complex solve of csrc/mg_krylov_host.hpp on its own.

The k x k solve is built into a stand-alone program (tests/native/complex_small_solve.cpp) with AddressSanitizer and
UndefinedBehaviorSanitizer, runtimes linked statically, and run as a child process; it is never loaded into Python.  Bound: 4 x 4
systems drawn until cond <= 100, Gaussian elimination with partial pivoting against numpy's LAPACK solve - k * cond * eps ~ 1e-13,
held to 1e-12 as tests/test_krylov_host_algebra.py holds the real instantiation."""
import os
import re
import subprocess

import numpy as np
import pytest

import complex_block_oracle as cb
import complex_krylov_oracle as ck
import complex_oracle as corc
from complex_cases import complex_rhs, helmholtz
from oracle import mg_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgvcycle.h")
SRC = os.path.join(ROOT, "tests", "native", "complex_small_solve.cpp")

ENTRY_POINTS = ["mg_block_spmv_CF64", "mg_block_cycle_CF64", "mg_block_solve_CF64", "mg_block_cycle_dev_CFP64", "mg_block_bicgstab_CFP64",
                "mg_block_bicgstab_dev_CFP64"]


def test_block_symbols_declared_exported_and_bound(mg, built):
    """Fails without the feature: the parent's header, library and binding have none of these."""
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(?:int|mg_status)\s+(mg_\w+)\s*\(", header))
    lib = mg.device.load_library()
    for n in ENTRY_POINTS:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in mg.device.SIGNATURES, n
    H = mg.device.ComplexDeviceHierarchy
    for n in ("block_spmv", "block_cycle", "block_solve", "block_cycle_dev", "block_bicgstab", "block_bicgstab_dev_CFP64"):
        assert callable(getattr(H, n)) and getattr(H, n) is not H._refuse, n
    for n in ("pcg", "block_pcg_dev", "block_fgmres_dev", "block_bicgstab_dev"):     # still refused (the last one: the FP64 method's name)
        assert getattr(H, n) is H._refuse, n
    assert callable(mg.solveBlockBiCGSTAB_MG_CFP64)


@pytest.mark.parametrize("relax,cyc,k", [("Jac", "V", 3), ("SPAI", "W", 2)])
def test_block_oracle_equals_real_block_oracle_on_real_data(mg, relax, cyc, k):
    """Real A, real B: conj is the identity and np.vdot a plain sum, so the complex block oracle runs the real one's operations.
    Same flag, count and resvec length; resvec and X within 1e-12 relative (the tolerance of the same pin for the vector drivers,
    tests/test_complex_krylov_host.py)."""
    A, mesh = mg.poisson_shifted([8, 8, 8])
    pr = mg.getMGparam(np.float64, np.int64, 2, 8, 30, 1e-8, relax, 0.8, 2, 1, cyc, "NoMUMPS", 0.5, 0.0)
    pc = mg.getMGparam(np.complex128, np.int64, 2, 8, 30, 1e-8, relax, 0.8, 2, 1, cyc, "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(A, mesh, pr)
    mg.MGsetup(A, mesh, pc)
    rng = np.random.default_rng(70 + k)
    B = np.asfortranarray(rng.standard_normal((A.shape[0], k)))
    Mr = orc.getMultigridPreconditioner(pr, B[:, 0].copy())
    Mblock = lambda V: np.stack([Mr(V[:, j].copy()).copy() for j in range(V.shape[1])], axis=1)
    xr, fr, itr, rvr = orc.blockBiCGSTB(lambda V: A @ V, B, 1e-8, 30, Mblock)
    xc, fc, itc, rvc = cb.blockBiCGSTB(lambda V: A @ V, B.astype(np.complex128), 1e-8, 30, cb.preconditioner(pc))
    assert (fr, itr, len(rvr)) == (fc, itc, len(rvc))
    assert fr in (0, -3) and itr > 1
    dr = np.abs(rvr - rvc).max() / rvr[0]
    dx = np.abs(xr - xc).max() / np.abs(xr).max()
    print(f"  resvec diff {dr:.2e}, x diff {dx:.2e}")
    assert dr <= 1e-12 and dx <= 1e-12
    assert np.abs(xc.imag).max() == 0.0


def test_block_solveMG_with_one_column_is_solveMG(mg):
    A, mesh = helmholtz(mg, [8, 8, 8], 0.5, 0.5)
    p = mg.getMGparam(np.complex128, np.int64, 2, 8, 6, 1e-8, "SPAI", 1.0, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(A, mesh, p)
    b = complex_rhs(A.shape[0], 31)
    h1, hb = {}, {}
    x1, it1 = corc.solveMG(p, b, np.zeros_like(b), h1)
    Xb, itb = cb.solveMG(p, b.reshape(-1, 1), np.zeros((b.size, 1), dtype=np.complex128), hb)
    assert it1 == itb and len(h1["resvec"]) == len(hb["resvec"])
    assert np.abs(h1["resvec"] - hb["resvec"]).max() <= 1e-14 * h1["resvec"][0]
    assert np.abs(Xb[:, 0] - x1).max() <= 1e-14 * np.abs(x1).max()


@pytest.mark.parametrize("name,k", sorted(cb.BLOCK_RUNS))
def test_block_oracle_counts_on_the_shared_cases(mg, name, k):
    """The (case, k) pairs the GPU test runs: the oracle converges, its count and flag are those of cb.BLOCK_RUNS, the entry that
    stops the run sits at least 4 % below tol and the one before it at least 1 % above (the guard of
    tests/test_complex_krylov_host.py), so a rounding difference on the device cannot move the stopping iteration."""
    p, As, _ = ck.case(mg, name)
    X, flag, it, rv = cb.reference(mg, name, k)
    B = cb.block_rhs(As.shape[0], k)
    print(f"  {name} k={k}: flag {flag}, count {it}, last entries {rv[-2]:.3e} {rv[-1]:.3e}")
    assert (it, flag) == cb.BLOCK_RUNS[(name, k)]
    assert len(rv) == 2 * it + (0 if flag == -3 else 1)
    assert rv[-1] < 0.96 * ck.TOL and rv[-2] > 1.01 * ck.TOL
    res = np.linalg.norm(B - As @ X, axis=0) / np.linalg.norm(B, axis=0)
    assert res.max() < ck.TOL


def test_complex_block_reaches_the_device_layer(mg, built):
    """A complex MGsolver("BiCGSTAB") given a block goes to solveBlockBiCGSTAB_MG_CFP64 and on to the device layer: without a GPU
    that is the library's own refusal (MGDeviceError), not the Python layer's NotImplementedError.  "GMRES" with a block stays refused."""
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    A, mesh = helmholtz(mg, [8, 8, 8], 0.5, 0.5)
    n = A.shape[0]
    B = cb.block_rhs(n, 3)

    def solver(krylov):
        p = mg.getMGparam(np.complex128, np.int64, 2, 8, 30, 1e-8, "SPAI", 1.0, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
        return mg.getMGsolver(p, mesh, 0, krylov)

    s = solver("GMRES")
    with pytest.raises(NotImplementedError):
        mg.solveLinearSystem_(A, B, np.zeros_like(B), s)
    mg.clear_(s.MG)
    s = solver("BiCGSTAB")
    X = np.zeros_like(B)
    if has_gpu:
        mg.solveLinearSystem_(A, B, X, s)
        assert np.linalg.norm(B - A @ X) / np.linalg.norm(B) < 1e-8
    else:
        with pytest.raises(mg.device.MGDeviceError):
            mg.solveLinearSystem_(A, B, X, s)
    mg.clear_(s.MG)


# ---- the k x k complex solve on its own -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("complex_small") / "complex_small_solve")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-o", exe, SRC], check=True, timeout=300)
    return exe


def _run(program, tmp_path, lines):
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(" ".join(repr(float(t)) if isinstance(t, (float, np.floating)) else str(t) for t in ln) for ln in lines) + "\n")
    p = subprocess.run([program, str(path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", f"exit {p.returncode}\n{p.stderr}"
    out = p.stdout.strip().split("\n")
    assert len(out) == len(lines) and all(o.split()[0] == ln[0] for o, ln in zip(out, lines))
    return [np.array([float(t) for t in o.split()[1:]]) for o in out]


def _pairs(M):
    M = np.asarray(M, dtype=np.complex128).ravel()
    return [float(v) for z in M for v in (z.real, z.imag)]


def _cx(out):
    return out[0::2] + 1j * out[1::2]


def _well_conditioned(rng, k, cx):
    while True:
        A = rng.standard_normal((k, k)) + (1j * rng.standard_normal((k, k)) if cx else 0.0)
        if np.linalg.cond(A) <= 100.0:
            return A


@pytest.mark.parametrize("seed", [5000, 5001, 5002])
def test_complex_small_solve_against_numpy(program, tmp_path, seed):
    rng = np.random.default_rng(seed)
    A = _well_conditioned(rng, 4, True)
    assert np.linalg.cond(A) <= 100.0
    B = rng.standard_normal((4, 3)) + 1j * rng.standard_normal((4, 3))
    (out,) = _run(program, tmp_path, [["solve_cx", 4, 3] + _pairs(A) + _pairs(B)])
    assert out[0] == 0.0
    X = _cx(out[1:]).reshape(4, 3)
    ref = np.linalg.solve(A, B)
    print(f"  cond {np.linalg.cond(A):.1f}: rel {np.linalg.norm(X - ref) / np.linalg.norm(ref):.2e}")
    assert np.linalg.norm(X - ref) <= 1e-12 * np.linalg.norm(ref)


def test_complex_small_solve_edges(program, tmp_path):
    rng = np.random.default_rng(5100)
    Ar = _well_conditioned(rng, 4, False)
    Br = rng.standard_normal((4, 2))
    M = rng.standard_normal((3, 3)) + 1j * rng.standard_normal((3, 3))
    v = 0.75 - 1.25j
    sing = np.array([[1.0 + 1j, 2.0], [2.0 + 2j, 4.0]])         # second row = 2 x the first: an exactly zero pivot
    re_out, cx_out, sing_out, ident = _run(program, tmp_path, [
        ["solve_re", 4, 2] + [float(t) for t in Ar.ravel()] + [float(t) for t in Br.ravel()],
        ["solve_cx", 4, 2] + _pairs(Ar) + _pairs(Br),
        ["solve_cx", 2, 1] + _pairs(sing) + _pairs([1.0, 1.0]),
        ["ident_cx", 3, float(v.real), float(v.imag)] + _pairs(M)])
    ref = np.linalg.solve(Ar, Br)
    # the double instantiation is untouched by the templating, and the complex one on real data takes the same pivots
    assert re_out[0] == 0.0 and np.linalg.norm(_cx(re_out[1:]).reshape(4, 2) - ref) <= 1e-12 * np.linalg.norm(ref)
    assert cx_out[0] == 0.0 and np.abs(_cx(cx_out[1:]).imag).max() == 0.0
    assert np.linalg.norm(_cx(cx_out[1:]).real.reshape(4, 2) - ref) <= 1e-12 * np.linalg.norm(ref)
    assert list(sing_out) == [1.0]                              # singular: refused, nothing written
    assert np.linalg.norm(_cx(ident).reshape(3, 3) - M * v) <= 1e-15 * np.linalg.norm(M * v) * 4
