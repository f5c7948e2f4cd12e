"""Complex block FGMRES, host side (no GPU): the block oracle (tests/complex_block_fgmres_oracle.py) pinned to the real block oracle and
to the single-vector complex FGMRES, the counts and guards the GPU tests rely on, the exported symbols, the Python surface, and the
complex small algebra of csrc/mg_krylov_host.hpp on its own.

The small algebra is built into a stand-alone program (tests/native/complex_block_lsq.cpp) with AddressSanitizer and
UndefinedBehaviorSanitizer, runtimes linked statically, and run as a child process; it is never loaded into Python.  Bounds: Gram
matrices of cond <= 1e4 and triangular factors of cond <= 1e2, so k * cond * eps stays below 1e-11 for the Cholesky factor (held to
1e-10) and below 1e-13 for the rest (held to 1e-12, as tests/test_complex_block_host.py holds the k x k solve)."""
import os
import re
import subprocess

import numpy as np
import pytest

import complex_block_fgmres_oracle as cf
import complex_block_oracle as cb
import complex_krylov_oracle as ck
from complex_cases import helmholtz
from oracle import mg_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgvcycle.h")
SRC = os.path.join(ROOT, "tests", "native", "complex_block_lsq.cpp")

ENTRY_POINTS = ["mg_block_fgmres_CFP64", "mg_block_fgmres_dev_CFP64", "mg_cblk_gram_dev_CFP64"]


def test_block_fgmres_symbols_declared_exported_and_bound(mg, built):
    """Fails without the feature: the parent's header, library and binding have none of these."""
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(?:int|mg_status)\s+(mg_\w+)\s*\(", header))
    lib = mg.device.load_library()
    for n in ENTRY_POINTS:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in mg.device.SIGNATURES, n
    assert mg.device.SIGNATURES["mg_block_fgmres_CFP64"] == mg.device.SIGNATURES["mg_block_fgmres_FP64"]
    assert mg.device.SIGNATURES["mg_block_fgmres_dev_CFP64"] == mg.device.SIGNATURES["mg_block_fgmres_dev_FP64"]
    H = mg.device.ComplexDeviceHierarchy
    for n in ("block_fgmres", "block_fgmres_dev_CFP64", "cblk_gram"):
        assert callable(getattr(H, n)) and getattr(H, n) is not H._refuse, n
    for n in ("pcg", "block_pcg_dev", "block_fgmres_dev", "block_bicgstab_dev"):     # still refused: the FP64 methods' names
        assert getattr(H, n) is H._refuse, n
    assert callable(mg.solveBlockGMRES_MG_CFP64) and "solveBlockGMRES_MG_CFP64" in mg.__all__


@pytest.mark.parametrize("relax,cyc,k,inner", [("Jac", "V", 3, 5), ("SPAI", "W", 2, 4)])
def test_block_fgmres_oracle_equals_real_block_oracle_on_real_data(mg, relax, cyc, k, inner):
    """Real A, real B: conj is the identity and np.vdot a plain sum, so the complex block oracle runs the real one's operations (the
    recipe of tests/test_complex_block_host.py).  Same flag, count and resvec length; resvec and X within 1e-12 relative."""
    A, mesh = mg.poisson_shifted([8, 8, 8])
    pr = mg.getMGparam(np.float64, np.int64, 2, 8, 30, 1e-8, relax, 0.8, 2, 1, cyc, "NoMUMPS", 0.5, 0.0)
    pc = mg.getMGparam(np.complex128, np.int64, 2, 8, 30, 1e-8, relax, 0.8, 2, 1, cyc, "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(A, mesh, pr)
    mg.MGsetup(A, mesh, pc)
    rng = np.random.default_rng(90 + k)
    B = np.asfortranarray(rng.standard_normal((A.shape[0], k)))
    Mr = orc.getMultigridPreconditioner(pr, B[:, 0].copy())
    Mblock = lambda V: np.stack([Mr(V[:, j].copy()).copy() for j in range(V.shape[1])], axis=1)
    xr, fr, itr, rvr = orc.blockFGMRES(lambda V: A @ V, B, inner, 1e-8, 30, Mblock)
    xc, fc, itc, rvc = cf.blockFGMRES(lambda V: A @ V, B.astype(np.complex128), inner, 1e-8, 30, cb.preconditioner(pc))
    assert (fr, itr, len(rvr)) == (fc, itc, len(rvc))
    assert fr == 0 and itr > inner                               # at least one restart
    dr = np.abs(rvr - rvc).max() / rvr[0]
    dx = np.abs(xr - xc).max() / np.abs(xr).max()
    print(f"  {itr} steps, resvec diff {dr:.2e}, x diff {dx:.2e}")
    assert dr <= 1e-12 and dx <= 1e-12
    assert np.abs(xc.imag).max() == 0.0


@pytest.mark.parametrize("name,k,inner", sorted(cf.BLOCK_FGMRES_RUNS))
def test_block_fgmres_oracle_counts_on_the_shared_cases(mg, name, k, inner):
    """The runs the GPU test repeats: the oracle converges with the count of cf.BLOCK_FGMRES_RUNS, the entry that stops the run sits
    more than 4 % below tol and the one before it more than 1 % above (the guard of tests/test_complex_krylov_host.py).
    cond(W^H W) of every Cholesky QR is printed and held below 1e13: Cholesky QR applied twice is orthonormal to rounding while
    cond(W) < eps^-1/2, cond(W^H W) < 1e16 (Yamamoto et al. 2015), and below 1e13 no pivot comes within a factor 10 of the cut at
    1e-14 G[c,c], so a device Gram matrix that differs by a few eps takes the same pivots.  Measured: 1.6e11 on (C3, 16, 5) - 80 of
    729 dimensions per restart, the blocks run short of new directions -, 2.1e4 on (C1, 4, 10), at most 20 on the others.
    The true residual is the one the method controls, ||B - A X||_F / ||B||_F (as tests/test_krylov.py checks blockFGMRES); the worst
    single column is printed: on (C1, 4, 10) the oracle itself leaves column 0 at 1.058e-8 with 8.10e-9 over the block."""
    p, As, _ = ck.case(mg, name)
    stats = []
    X, flag, steps, rv = cf.reference(mg, name, k, inner, stats=stats)
    B = cb.block_rhs(As.shape[0], k)
    print(f"  {name} k={k} inner={inner}: flag {flag}, steps {steps}, last entries {rv[-2]:.3e} {rv[-1]:.3e}, worst cond {max(stats):.1f}")
    assert flag == 0 and steps == cf.BLOCK_FGMRES_RUNS[(name, k, inner)] and len(rv) == steps
    assert rv[-1] < 0.96 * ck.TOL and rv[-2] > 1.01 * ck.TOL
    assert max(stats) < 1e13
    print(f"    true residual {np.linalg.norm(B - As @ X) / np.linalg.norm(B):.3e} over the block, "
          f"{(np.linalg.norm(B - As @ X, axis=0) / np.linalg.norm(B, axis=0)).max():.3e} in the worst column")
    assert np.linalg.norm(B - As @ X) / np.linalg.norm(B) < ck.TOL


def test_block_fgmres_oracle_with_one_column_against_fgmres(mg):
    """k = 1: the block method (Cholesky QR, Householder least squares) and ck.fgmres (normalisation, Givens rotations) are the same
    method in exact arithmetic but differ in their orthogonalisation, so iterates are not compared: both converge and their true
    relative residuals agree to within tol."""
    p, As, _ = ck.case(mg, "C3")
    X, flag, steps, rv = cf.reference(mg, "C3", 1, 5)
    b = cb.block_rhs(As.shape[0], 1)[:, 0]
    x, f1, s1, rv1 = ck.fgmres(lambda v: As @ v, b, 5, ck.TOL, ck.MAXIT_FGMRES, ck.preconditioner(p))
    rb = np.linalg.norm(b - As @ X[:, 0]) / np.linalg.norm(b)
    r1 = np.linalg.norm(b - As @ x) / np.linalg.norm(b)
    print(f"  block: {steps} steps, residual {rb:.3e}; fgmres: {s1} steps, residual {r1:.3e}")
    assert flag == 0 and f1 == 0
    assert rb < ck.TOL and r1 < ck.TOL and abs(rb - r1) <= ck.TOL


def test_complex_block_gmres_reaches_the_device_layer(mg, built):
    """solveBlockGMRES_MG_CFP64 goes to the device layer: without a GPU that is the library's own refusal (MGDeviceError), not the
    Python layer's NotImplementedError; the pinned refusals around it stay."""
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    A, mesh = helmholtz(mg, [8, 8, 8], 0.5, 0.5)
    n = A.shape[0]
    B = cb.block_rhs(n, 3)
    p = mg.getMGparam(np.complex128, np.int64, 2, 8, 20, 1e-8, "SPAI", 1.0, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(A, mesh, p)
    try:
        X = np.zeros_like(B)
        if has_gpu:
            Xr, q, steps, rv = mg.solveBlockGMRES_MG_CFP64(A, p, B, X, True, 5)
            assert Xr is X and q is p and p.flag == 0 and len(rv) == steps
            assert np.linalg.norm(B - A @ X) / np.linalg.norm(B) < 1e-8
        else:
            with pytest.raises(mg.device.MGDeviceError):
                mg.solveBlockGMRES_MG_CFP64(A, p, B, X, True, 5)
        with pytest.raises(NotImplementedError):                   # the single-vector function given a block stays refused
            mg.solveGMRES_MG_CFP64(A, p, B, np.zeros_like(B), True, 5)
        with pytest.raises(TypeError):
            pr = mg.getMGparam(np.float64, np.int64, 2, 8, 20, 1e-8, "Jac", 0.8, 2, 1, "V")
            mg.solveBlockGMRES_MG_CFP64(None, pr, B.real.copy(), np.zeros((n, 3)), True, 5)
    finally:
        mg.clear_(p)


# ---- the complex small algebra on its own ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("complex_block_lsq") / "complex_block_lsq")
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


def _block_of_cond(rng, n, k, cond):
    """n x k complex block whose Gram matrix has the given condition number."""
    Q, _ = np.linalg.qr(rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k)))
    U, _ = np.linalg.qr(rng.standard_normal((k, k)) + 1j * rng.standard_normal((k, k)))
    return Q @ np.diag(np.geomspace(1.0, 1.0 / np.sqrt(cond), k)) @ U.conj().T


def test_complex_chol_semidefinite_and_tri_pinv(program, tmp_path):
    rng = np.random.default_rng(6000)
    k = 5
    W = _block_of_cond(rng, 40, k, 1e4)
    G = W.conj().T @ W
    # rank deficient: column 2 = a combination of columns 0 and 1, column 4 = zero (on a block of cond(G) = 16, so that the
    # rounding of the dependent column's pivot, a few eps * cond * G[c,c], stays well below the cut at 1e-14 * G[c,c])
    Wd = _block_of_cond(rng, 40, k, 16.0)
    Wd[:, 2] = (0.5 - 1.5j) * Wd[:, 0] + (2.0 + 0.25j) * Wd[:, 1]
    Wd[:, 4] = 0.0
    Gd = Wd.conj().T @ Wd
    Gr = (W.real.T @ W.real)
    full, defi, re_cx, re_re = _run(program, tmp_path, [["chol_cx", k] + _pairs(G), ["chol_cx", k] + _pairs(Gd),
                                                       ["chol_cx", k] + _pairs(Gr), ["chol_re", k] + [float(t) for t in Gr.ravel()]])
    R = _cx(full).reshape(k, k)
    assert np.abs(np.tril(R, -1)).max() == 0.0 and np.abs(np.diag(R).imag).max() == 0.0 and np.diag(R).real.min() > 0.0
    e = np.linalg.norm(R.conj().T @ R - G) / np.linalg.norm(G)
    ref = np.linalg.cholesky(G).conj().T                         # the unique factor with a positive diagonal
    print(f"  cond(G) {np.linalg.cond(G):.1e}: ||R^H R - G|| {e:.2e}, against LAPACK {np.linalg.norm(R - ref) / np.linalg.norm(ref):.2e}")
    assert e <= 1e-14 and np.linalg.norm(R - ref) <= 1e-10 * np.linalg.norm(ref)
    assert np.linalg.norm(R - cf._chol_semidefinite(G)) <= 1e-10 * np.linalg.norm(R)
    Rd = _cx(defi).reshape(k, k)
    assert not Rd[2].any() and not Rd[4].any()                   # the dependent and the zero column are dropped: zero rows
    assert Rd[0, 0].real > 0 and Rd[1, 1].real > 0 and Rd[3, 3].real > 0
    assert np.linalg.norm(Rd.conj().T @ Rd - Gd) <= 1e-12 * np.linalg.norm(Gd)
    assert np.linalg.norm(Rd - cf._chol_semidefinite(Gd)) <= 1e-10 * np.linalg.norm(Rd)
    # real data: the complex form takes the real form's pivots and values
    assert np.abs(_cx(re_cx).imag).max() == 0.0 and np.array_equal(_cx(re_cx).real, _cx(re_re).real)
    # tri_pinv: W T = W R^+ on the full factor (T = R^-1) and on the deficient one (zero columns at the dropped pivots)
    Rw = np.triu(rng.standard_normal((k, k)) + 1j * rng.standard_normal((k, k)), 1) + np.diag(np.linspace(1.0, 2.0, k))
    assert np.linalg.cond(Rw) <= 100.0
    t_full, t_def = _run(program, tmp_path, [["tripinv_cx", k] + _pairs(Rw), ["tripinv_cx", k] + _pairs(Rd)])
    T = _cx(t_full).reshape(k, k)
    assert np.linalg.norm(T - np.linalg.inv(Rw)) <= 1e-12 * np.linalg.norm(np.linalg.inv(Rw))
    Td = _cx(t_def).reshape(k, k)
    assert not Td[:, 2].any() and not Td[:, 4].any()
    Qo = cf._tri_pinv_apply(Wd, Rd)
    assert np.linalg.norm(Wd @ Td - Qo) <= 1e-12 * np.linalg.norm(Qo)
    Gq = (Wd @ Td).conj().T @ (Wd @ Td)
    assert np.linalg.norm(Gq - np.diag([1, 1, 0, 1, 0])) <= 1e-10  # orthonormal on the kept columns


@pytest.mark.parametrize("j,k", [(0, 1), (2, 3), (4, 2)])
def test_complex_block_hessenberg_lstsq_against_numpy(program, tmp_path, j, k):
    """min ||xi - H Y||_F on a (j+2)k x (j+1)k block upper Hessenberg matrix with triangular sub-diagonal blocks, as the driver's
    inner step j poses it, against numpy's lstsq."""
    rng = np.random.default_rng(6100 + 10 * j + k)
    m, n = (j + 2) * k, (j + 1) * k
    H = rng.standard_normal((m, n)) + 1j * rng.standard_normal((m, n))
    for c in range(j + 1):
        H[(c + 2) * k:, c * k:(c + 1) * k] = 0.0
        H[(c + 1) * k:(c + 2) * k, c * k:(c + 1) * k] = np.triu(H[(c + 1) * k:(c + 2) * k, c * k:(c + 1) * k]) + 2.0 * np.eye(k)
    xi = np.zeros((m, k), dtype=np.complex128)
    xi[:k] = np.triu(rng.standard_normal((k, k)) + 1j * rng.standard_normal((k, k)))
    assert np.linalg.cond(H) <= 100.0
    (out,) = _run(program, tmp_path, [["lstsq_cx", m, n, k] + _pairs(H) + _pairs(xi)])
    res, Y = out[0], _cx(out[2:]).reshape(n, k)
    Yo = np.linalg.lstsq(H, xi, rcond=None)[0]
    ro = np.linalg.norm(xi - H @ Yo)
    print(f"  {m} x {n}, cond {np.linalg.cond(H):.1f}: Y rel {np.linalg.norm(Y - Yo) / np.linalg.norm(Yo):.2e}, residual {res:.6e} ({ro:.6e})")
    assert out[1] == 0.0
    assert np.linalg.norm(Y - Yo) <= 1e-12 * np.linalg.norm(Yo)
    assert abs(res - ro) <= 1e-12 * np.linalg.norm(xi)
