"""-m "not gpu": the host side of the GMRES coarsest solve of complex hierarchies (coarseSolveType = "GMRES").

1. The oracle pin.  tests/complex_coarse_cases.py's coarsest solve inside tests/complex_oracle.py on a REAL shifted-Poisson hierarchy cast
   to complex equals oracle/mg_oracle.py's real GMRES coarse solve: two cycles within 1e-12 of max|x| (the pin tests/test_complex_kcycle_host.py
   uses for its branches).
2. The table replay (coarse_gmres_replay of csrc/mg_krylov_host.hpp) on its own.  tests/native/coarse_gmres_replay.cpp includes nothing but
   that header; it is built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process, exactly as
   tests/test_complex_kcycle_host.py runs relax_lsq_complex.cpp.  The table is written here from a plain numpy Arnoldi process (all 10
   steps, as the device runs them); `used`, the estimates and y must be the oracle's: the estimates to 1e-13 relative, y (recovered from
   the oracle's x = Z[:, :used] y by least squares) to 1e-10 relative - y goes through a triangular solve with H, whose condition stays
   below 1e3 on these cases.
3. The library exports the two new symbols; a cycle on such a param reaches the device layer; a block of two columns is refused by the
   Python layer before the device is touched.  (Without a GPU the device layer's refusal is mg_create's "no device", which comes ahead
   of the coarse setter: what fails without the feature are the symbols and the block refusal here, and every GPU test.)"""
import os
import subprocess

import numpy as np
import pytest

import complex_coarse_cases as cc
import complex_krylov_oracle as ck
import complex_oracle as corc
from complex_cases import complex_rhs
from oracle import mg_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "coarse_gmres_replay.cpp")


# ---- 1. the oracle pin -------------------------------------------------------------------------------------------------------------
def test_oracle_on_real_operator_equals_real_oracle(mg):
    A, mesh = mg.poisson_shifted([8, 8, 8])
    pr = mg.getMGparam(np.float64, np.int64, 3, 8, 4, 1e-10, "Jac", 0.8, 2, 1, "V", "GMRES", 0.5, 0.0)
    mg.MGsetup(A, mesh, pr)
    assert isinstance(pr.LU, np.ndarray) and pr.LU.shape == (pr.As[-1].shape[0],)
    import copy
    pc = copy.copy(pr)
    pc.As = [M.astype(np.complex128) for M in pr.As]
    pc.relaxPrecs = [np.asarray(d, dtype=np.complex128) for d in pr.relaxPrecs]
    pc.LU = cc.OracleCoarseGmres(pc.As[-1], pr.LU)
    pc.device = None
    b = mg.seeded_rhs(A)
    xr = orc.recursiveCycle(pr, b, np.zeros_like(b), 1).copy()
    xc = corc.recursiveCycle(pc, b.astype(np.complex128), np.zeros(b.size, dtype=np.complex128), 1).copy()
    print(f"first cycle: {np.abs(xc - xr).max() / np.abs(xr).max():.2e}")
    assert np.abs(xc - xr).max() <= 1e-12 * np.abs(xr).max()
    xr = orc.recursiveCycle(pr, b, xr, 1).copy()
    xc = corc.recursiveCycle(pc, b.astype(np.complex128), xc, 1).copy()
    print(f"second cycle: {np.abs(xc - xr).max() / np.abs(xr).max():.2e}; coarsest solves {[(f, s) for f, s, _ in pc.LU.log]}")
    assert np.abs(xc - xr).max() <= 1e-12 * np.abs(xr).max()
    assert len(pc.LU.log) == 2 and all(1 <= s <= 10 for _, s, _ in pc.LU.log)
    mg.clear_(pr)


# ---- 2. the table replay -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("coarse_gmres_replay") / "coarse_gmres_replay")
    # (the sanitizers' runtimes are linked statically: the program then runs whatever libraries the caller's environment loads ahead of it)
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


def _slot(i):
    return 1 + i * i + 2 * i


def _table(A, d, b, m=10):
    """The scalar table of a whole restart (no break: the device runs every step) and Z: ||b||^2, then per step h_0 .. h_i, ||w||^2."""
    tab = np.zeros((m + 1) ** 2)
    bn2 = np.vdot(b, b).real
    tab[0] = bn2
    V = [b / np.sqrt(bn2)]
    Z = []
    for i in range(m):
        Z.append(d * V[i])
        w = A @ Z[i]
        for k in range(i + 1):
            h = np.vdot(V[k], w)
            w = w - h * V[k]
            tab[_slot(i) + 2 * k], tab[_slot(i) + 2 * k + 1] = h.real, h.imag
        wn2 = np.vdot(w, w).real
        tab[_slot(i) + 2 * (i + 1)] = wn2
        V.append(w / np.sqrt(wn2) if wn2 > 0 else np.zeros_like(w))
    return tab, np.array(Z).T


def _parse(out):
    used, flag = int(out[0]), int(out[1])
    res = out[2:2 + used]
    y = out[2 + used:2 + 3 * used]
    return used, flag, res, y[0::2] + 1j * y[1::2]


@pytest.mark.parametrize("name", ["awkward5000_f0.3", "S100_f1.5"])
def test_replay_reproduces_the_oracle(program, tmp_path, name):
    A, d, b, orc_solve, xo = cc.solve_case(name)
    flag_o, steps_o, res_o = orc_solve.log[0]
    assert cc.clearance(orc_solve.log) >= cc.MIN_CLEARANCE
    assert (steps_o, flag_o == 0) == cc.solve_expected(name)          # no break / a break at step 4
    tab, Z = _table(A, d, b)
    used, flag, res, y = _parse(_run(program, tmp_path, [["replay", 10, 0.01] + list(tab)])[0])
    assert used == steps_o and flag == flag_o
    assert np.abs(res - res_o).max() <= 1e-13 * np.abs(res_o).max()
    yo = np.linalg.lstsq(Z[:, :used], xo, rcond=None)[0]
    print(f"{name}: used {used} flag {flag}  estimates {np.abs(res - res_o).max() / np.abs(res_o).max():.2e}  y {np.abs(y - yo).max() / np.abs(yo).max():.2e}")
    assert np.abs(y - yo).max() <= 1e-10 * np.abs(yo).max()
    assert np.abs(Z[:, :used] @ y - xo).max() <= 1e-12 * np.abs(xo).max()


def test_replay_zero_right_hand_side(program, tmp_path):
    out = _run(program, tmp_path, [["replay", 10, 0.01] + [0.0] * 121])[0]
    assert list(out) == [0.0, -9.0]                                     # used = 0, flag -9, nothing else: x = 0
    x, flag, steps, res = ck.fgmres(lambda v: v, np.zeros(5, dtype=np.complex128), 10, 0.01, 1)
    assert flag == -9 and steps == 0 and not x.any()


def test_replay_zero_w_column(program, tmp_path):
    """||w|| = 0 behind the first step (A z_0 = h_0 v_0 exactly): the column closes with sine 0, the estimate is 0, the loop breaks,
    y_0 = ||b|| / h_0.  The steps behind it ran on zero vectors: their scalars are zeros and are not read."""
    h0, bn = 0.8 + 0.1j, 2.0
    tab = np.zeros(121)
    tab[0] = bn * bn
    tab[1], tab[2] = h0.real, h0.imag
    used, flag, res, y = _parse(_run(program, tmp_path, [["replay", 10, 0.01] + list(tab)])[0])
    assert used == 1 and flag == 0 and res[0] == 0.0
    assert np.isfinite(y).all() and abs(y[0] - bn / h0) <= 1e-15 * abs(bn / h0)


# ---- 3. symbols, the first layer, blocks ---------------------------------------------------------------------------------------------
def test_library_exports_the_coarse_gmres_symbols(mg, built):
    lib = mg.device.load_library()
    for name in ("mg_set_coarse_gmres_CF64", "mg_coarse_gmres_CF64"):
        assert hasattr(lib, name) and name in mg.device.SIGNATURES


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_complex_gmres_coarse_reaches_the_device_layer(mg, built):
    """recursiveCycle on a complex GMRES-coarse param is not refused by the Python layer (no NotImplementedError): without a GPU it
    ends in the library's own refusal (MGDeviceError), with one it runs."""
    p = cc.hierarchy(mg, "3lev")
    assert p.coarseSolveType == "GMRES" and isinstance(p.LU, np.ndarray) and p.LU.dtype == np.complex128
    assert np.abs(p.LU - 0.8 / p.As[-1].diagonal()).max() == 0.0
    b = cc.cycle_rhs(p)
    x = np.zeros_like(b)
    if _has_gpu():
        mg.recursiveCycle(p, b, x, 1)
        assert np.isfinite(x).all() and np.abs(x).max() > 0
    else:
        with pytest.raises(mg.device.MGDeviceError):
            mg.recursiveCycle(p, b, x, 1)
    mg.clear_(p)


def test_block_on_complex_gmres_coarse_is_refused(mg, built):
    p = cc.hierarchy(mg, "3lev")
    n = p.As[0].shape[0]
    B = np.asfortranarray(np.stack([complex_rhs(n, 9), complex_rhs(n, 10)], axis=1))
    for call in (lambda: mg.recursiveCycle(p, B, np.zeros_like(B), 1), lambda: mg.solveMG(p, B, np.zeros_like(B)),
                 lambda: mg.getMultigridPreconditioner(p, B), lambda: mg.solveBlockBiCGSTAB_MG_CFP64(None, p, B, np.zeros_like(B))):
        with pytest.raises(NotImplementedError):
            call()
    assert p.device is None                                            # refused before the device is touched
    mg.clear_(p)
