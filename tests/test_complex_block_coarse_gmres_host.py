"""-m "not gpu": the block GMRES coarsest solve of complex hierarchies (blockFGMRES in solveCoarsest, MGcycle.jl:165-167) as far as a
host can check it.

1. The oracles.  At k = 1 the block oracle (complex_block_coarse_cases.OracleBlockCoarseGmres) takes the steps of the single-vector one
   (complex_coarse_cases.OracleCoarseGmres) with estimates within 1e-12.  The runs of the shared cases take the steps and flags their
   tables state, with a clearance of 1.5 from the stopping threshold.  The whole-block cycle is not the column-by-column cycle: on the
   two-level case the two differ by far more than the 1e-11 the device is held to.
2. The noise run behind the GPU tolerances: relative noise of 1e-13 on every A_c Z_j must move X and the estimates of every case by less
   than a quarter of its tolerance (1e-11 / 1e-10), or the case is wrong.
3. The table replay (coarse_block_gmres_replay / BlockHessenbergLsq of csrc/mg_krylov_host.hpp) on its own.
   tests/native/coarse_block_gmres_replay.cpp includes nothing but that header; it is built with AddressSanitizer and
   UndefinedBehaviorSanitizer and run as a child process.  The table is written here from a numpy block Arnoldi process with the oracle's
   own Cholesky QR (all 10 steps, as the device runs them); `used`, flag and the estimates must be the oracle's (1e-12 relative), and
   sum_j Z_j Y_j its X (1e-11: Y goes through a triangular solve with H).  The banded Householder route must agree with sm_lstsq on the
   leading blocks, the block FGMRES driver's route (it adds exact zeros to the same sums: 1e-14).  The zero-column case included.
4. The library exports the new symbols; getMGparam / copySolver carry blockCoarseGMRES; without it the Python layer refuses a block
   before the device is touched, with it the block reaches the device layer (MGDeviceError without a GPU)."""
import os
import subprocess

import numpy as np
import pytest

import complex_block_coarse_cases as cbc
import complex_block_fgmres_oracle as bf
import complex_block_oracle as cb
import complex_coarse_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "coarse_block_gmres_replay.cpp")


# ---- 1. the oracles ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.SOLVE_CASES)
def test_block_oracle_of_one_column_is_the_vector_oracle(name):
    A, d, b, orc1, xo = cc.solve_case(name)
    orc = cbc.OracleBlockCoarseGmres(A, d)
    x = orc.solve(b)
    (f1, s1, r1), (fb, sb, rb) = orc1.log[0], orc.log[0]
    assert (fb, sb) == (f1, s1)
    assert np.abs(rb - r1).max() <= 1e-12 * np.abs(r1).max()
    assert np.abs(x - xo).max() <= 1e-11 * np.abs(xo).max()


@pytest.mark.parametrize("name,k", sorted(cbc.SOLVE_RUNS))
def test_shared_solves_take_the_stated_steps(name, k):
    A, d, B, orc, X = cbc.solve_case(name, k)
    flag, steps, res = orc.log[0]
    print(f"{name} k={k}: steps {steps} flag {flag} clearance {cbc.clearance(orc.log):.2f}")
    assert (steps, flag) == cbc.SOLVE_RUNS[(name, k)]
    assert cbc.clearance(orc.log) >= cbc.MIN_CLEARANCE


def test_zero_column_gives_an_exactly_zero_column():
    name, k = cbc.ZERO_COLUMN
    A, d, B, orc, X = cbc.solve_case(name, k, zero_column=True)
    flag, steps, res = orc.log[0]
    assert (steps, flag) == (4, 0) and cbc.clearance(orc.log) >= cbc.MIN_CLEARANCE
    assert not B[:, 1].any() and not X[:, 1].any() and X[:, 0].any() and X[:, 2].any()


def test_whole_block_cycle_is_not_the_column_by_column_cycle(mg):
    p = cbc.hierarchy(mg, "16_2lev")
    B = cbc.cycle_rhs(p, 4)
    q = cbc.oracle_param(p)
    Xw = cbc.block_cycle(q, B, np.zeros_like(B))
    assert cbc.clearance(q.LU.log) >= cbc.MIN_CLEARANCE
    qc = cc.oracle_param(p)                                            # the single-vector coarsest solve, column by column
    Xc = cb.block_cycle(qc, B, np.zeros(B.shape, dtype=np.complex128))
    diff = np.abs(Xw - Xc).max() / np.abs(Xw).max()
    print(f"whole block against column by column: {diff:.2e}")
    assert diff > 1e-6                                                 # (the device is held to 1e-11 against the whole-block oracle)
    # one column through the whole-block cycle IS the vector cycle
    q1 = cbc.oracle_param(p)
    x1 = cbc.block_cycle(q1, B[:, :1], np.zeros((B.shape[0], 1), dtype=np.complex128))
    assert np.abs(x1[:, 0] - Xc[:, 0]).max() <= 1e-11 * np.abs(Xc[:, 0]).max()
    mg.clear_(p)


# ---- 2. the noise run -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("awkward5000_f0.3", 2), ("awkward5000_f0.3", 16), ("awkward5000_f1.5", 3), ("awkward5000_f1.5", 16),
                                    ("S100_f1.5", 2), ("S100_f1.5", 8)])
def test_noise_of_1e_13_stays_below_a_quarter_of_the_tolerances(name, k):
    A, d, B, orc, X0 = cbc.solve_case(name, k)
    _, s0, r0 = orc.log[0]
    rng = np.random.default_rng(0)
    worst_x = worst_r = 0.0
    for _ in range(3):
        noisy = cbc.OracleBlockCoarseGmres(A, d)
        noisy.afun = lambda V: (A @ V) * (1 + 1e-13 * rng.standard_normal(V.shape))
        X1 = noisy.solve(B)
        _, s1, r1 = noisy.log[0]
        assert s1 == s0
        worst_x = max(worst_x, np.abs(X1 - X0).max() / np.abs(X0).max())
        worst_r = max(worst_r, np.abs(r1 - r0).max() / np.abs(r0).max())
    print(f"{name} k={k}: X moved {worst_x:.2e}, estimates moved {worst_r:.2e}")
    assert worst_x <= 0.25 * 1e-11 and worst_r <= 0.25 * 1e-10


# ---- 3. the replay --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("coarse_block_gmres_replay") / "coarse_block_gmres_replay")
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


def _slot(j):
    return 1 + j * (j + 3) // 2


def _table(A, d, B, m=10):
    """The table of a whole restart (no break: the device runs every step) and the blocks Z_j: ||B||_F^2, a pad, xi_0, then per step
    H_0j .. H_jj, H_{j+1,j} - k x k complex blocks, row-major.  The Cholesky QR is the oracle's own."""
    n, k = B.shape
    blocks = np.zeros((_slot(m), k, k), dtype=np.complex128)
    V = [None] * (m + 1)
    Z = []
    V[0], blocks[0] = bf._cholqr(np.array(B, dtype=np.complex128))
    for j in range(m):
        Z.append(d[:, None] * V[j])
        W = A @ Z[j]
        for i in range(j + 1):
            Hij = V[i].conj().T @ W
            blocks[_slot(j) + i] = Hij
            W = W - V[i] @ Hij
        V[j + 1], blocks[_slot(j) + j + 1] = bf._cholqr(W)
    tab = np.zeros(2 + 2 * blocks.size)
    tab[0] = np.linalg.norm(B) ** 2
    tab[2::2], tab[3::2] = blocks.real.ravel(), blocks.imag.ravel()
    return tab, Z


def _parse(out, k):
    used, flag = int(out[0]), int(out[1])
    res = out[2:2 + used]
    y = out[2 + used:2 + used + 2 * used * k * k]
    Y = (y[0::2] + 1j * y[1::2]).reshape(used * k, k)
    return used, flag, res, Y, out[-2], out[-1]


@pytest.mark.parametrize("name,k,zero", [("awkward5000_f0.3", 2, False), ("awkward5000_f1.5", 5, False), ("awkward5000_f1.5", 16, False),
                                         ("S100_f1.5", 3, False), ("S100_f1.5", 8, False), ("S100_f1.5", 3, True)])
def test_replay_reproduces_the_oracle(program, tmp_path, name, k, zero):
    A, d, B, orc, Xo = cbc.solve_case(name, k, zero_column=zero)
    flag_o, steps_o, res_o = orc.log[0]
    assert cbc.clearance(orc.log) >= cbc.MIN_CLEARANCE
    tab, Z = _table(A, d, B)
    assert len(tab) == 2 + 2 * k * k * _slot(10)
    used, flag, res, Y, dres, dY = _parse(_run(program, tmp_path, [["replay", k, 10, 0.01] + list(tab)])[0], k)
    assert used == steps_o and flag == flag_o
    er = np.abs(res - res_o).max() / np.abs(res_o).max()
    X = sum(Z[j] @ Y[j * k:(j + 1) * k] for j in range(used))
    ex = np.abs(X - Xo).max() / np.abs(Xo).max()
    print(f"{name} k={k} zero={zero}: used {used} flag {flag}  estimates {er:.2e}  X {ex:.2e}  against sm_lstsq: residual {dres:.2e} Y {dY:.2e}")
    assert er <= 1e-12 and ex <= 1e-11
    assert dres <= 1e-14 and dY <= 1e-12 * np.abs(Y).max()
    if zero:
        assert not X[:, 1].any()                                       # exact zeros: the dropped column's rows of H and xi_0 are zero


def test_replay_zero_right_hand_side(program, tmp_path):
    k = 3
    out = _run(program, tmp_path, [["replay", k, 10, 0.01] + [0.0] * (2 + 2 * k * k * _slot(10))])[0]
    assert list(out) == [0.0, -9.0, 0.0, 0.0]                          # used = 0, flag -9, no estimates, no Y: X = 0
    X, flag, steps, res = bf.blockFGMRES(lambda V: V, np.zeros((5, k), dtype=np.complex128), 10, 0.01, 1)
    assert flag == -9 and steps == 0 and not X.any()


# ---- 4. symbols and the Python layer ------------------------------------------------------------------------------------------------------
def test_library_exports_the_block_coarse_gmres_symbols(mg, built):
    lib = mg.device.load_library()
    for name in ("mg_block_coarse_gmres_CF64", "mg_block_coarse_form"):
        assert hasattr(lib, name) and name in mg.device.SIGNATURES


def test_param_carries_the_opt_in(mg):
    p = mg.getMGparam(np.complex128, np.int64, 3, 8, 8, 1e-10, "Jac", 0.8, 2, 1, "V", "GMRES", 0.5, 0.0, blockCoarseGMRES=True)
    assert p.blockCoarseGMRES is True and mg.copySolver(p).blockCoarseGMRES is True
    ps = mg.getMGparam(np.complex128, np.int64, 3, 8, 8, 1e-10, "Jac", 0.8, 2, 1, "V", "GMRES", 0.5, 0.0, singlePrecision=True,
                       blockCoarseGMRES=True)
    assert ps.blockCoarseGMRES and ps.singlePrecision and mg.copySolver(ps).blockCoarseGMRES
    assert mg.getMGparam(np.complex128, np.int64, 3, 8, 8, 1e-10, "Jac", 0.8, 2, 1, "V", "GMRES").blockCoarseGMRES is False
    with pytest.raises(TypeError):                                     # keyword only
        mg.getMGparam(np.complex128, np.int64, 3, 8, 8, 1e-10, "Jac", 0.8, 2, 1, "V", "GMRES", 0.5, 0.0, "FullWeighting", False, True)
    with pytest.raises(NotImplementedError):                           # a real param, another coarsest solve
        mg.getMGparam(np.float64, np.int64, 3, 8, 8, 1e-10, "Jac", 0.8, 2, 1, "V", "GMRES", blockCoarseGMRES=True)
    with pytest.raises(NotImplementedError):
        mg.getMGparam(np.complex128, np.int64, 3, 8, 8, 1e-10, "Jac", 0.8, 2, 1, "V", "NoMUMPS", blockCoarseGMRES=True)


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_block_is_refused_without_the_opt_in_and_reaches_the_device_with_it(mg, built):
    p0 = cbc.hierarchy(mg, "16_3levV", opt_in=False)
    B = cbc.cycle_rhs(p0, 2)
    calls = lambda p: (lambda: mg.recursiveCycle(p, B, np.zeros_like(B), 1), lambda: mg.solveMG(p, B, np.zeros_like(B)),
                       lambda: mg.getMultigridPreconditioner(p, B), lambda: mg.solveBlockBiCGSTAB_MG_CFP64(None, p, B, np.zeros_like(B)),
                       lambda: mg.solveBlockGMRES_MG_CFP64(None, p, B, np.zeros_like(B), True, 5),
                       lambda: mg.SpMatMul(p, 1, "A", B, np.zeros_like(B)))
    for call in calls(p0):
        with pytest.raises(NotImplementedError):
            call()
    assert p0.device is None                                           # refused before the device is touched
    mg.clear_(p0)
    p = cbc.hierarchy(mg, "16_3levV")
    assert p.blockCoarseGMRES
    for call in calls(p):
        if _has_gpu():
            call()
        else:
            with pytest.raises(mg.device.MGDeviceError):
                call()
    if _has_gpu():
        X = np.zeros_like(B)
        mg.recursiveCycle(p, B, X, 1)
        assert np.isfinite(X).all() and np.abs(X).max() > 0 and p.device.block_coarse_form(2)["served"]
    mg.clear_(p)
