"""Shared by the tests of blocks of right-hand sides on complex Vanka hierarchies (``getMGparam(..., complexVanka=True,
vankaBlocks=True)``): the cases, their flagged hierarchies, the blocks, and the block restatement - the column loop over
``vanka_cases.restate_relax`` / ``complex_vanka_cases.restate_cycle`` (the smoother and the cycle are column-separable; the one
thing a block decides as a whole is ``norm(x) > 0``, and a zero column run through the general path takes the values of the
from-zero path).  Imports no device code of the package and changes nothing of the modules it imports.

Residual factors (Frobenius norms of the block) of two cycles of the block restatement, one from zero and one from the iterate,
on the blocks with one all-zero column (asserted < 0.5 by tests/test_complex_vanka_block_host.py::
test_block_restatement_contracts) are recorded in ``FACTORS`` below, for k = 3 and k = 16; five cycles of 24v, k = 3 (the block
solveMG case): 0.141 0.212 0.227 0.254 0.298.

The drivers' problem is the lightly damped operator of tests/test_complex_vanka_gpu.py::test_drivers, rebuilt here
(``helmholtz_K``): K = A_real - omega^2 (1 - 0.01i) S on [32, 32], preconditioned by one cycle of the hierarchy built on the
0.1-damped operator.  ``DRIVER_STEPS`` records the inner steps ``complex_block_fgmres_oracle.blockFGMRES`` (inner 5, tol 1e-8, at
most 10 restarts = 50 steps) takes on the k = 3 block with M = the column-wise restatement, CF64 and CF32 (the mixed closure);
test_driver_oracle_counts runs the oracle on the CPU and asserts them, flag 0 and the true residual, so the GPU bound tests the
device and not the problem."""
import numpy as np
import scipy.sparse as sp

import complex_block_fgmres_oracle as bf
import complex_vanka_cases as CV
import vanka_cases as V

KMAX = 16
# id -> (case of complex_vanka_cases.CASES, options of param)
BLOCK_CYCLES = {"24v": ("24v", {}), "24w": ("24w", {}), "12v": ("12v", {}), "24f": ("24v", {"cycle": "F"})}
# stand-alone smoother: (cells, includePressure) - bs 7 with 120 cells per colour (a partial workgroup); bs 5; 6 cells per colour
# (less than one wavefront at k = 1); bs 6
SMOOTHER_SHAPES = [([12, 8, 10], True), ([24, 16], True), ([6, 4], True), ([12, 8, 10], False)]
SMOOTHER_K = [1, 3, 16]          # 3: wavefronts straddle cells
# (case, k) -> the two residual factors of the block restatement (measured on the CPU, asserted to 2e-3)
FACTORS = {("24v", 3): (0.141, 0.212), ("24v", 16): (0.137, 0.214), ("24w", 3): (0.138, 0.209), ("24w", 16): (0.134, 0.209),
           ("12v", 3): (0.142, 0.240), ("12v", 16): (0.142, 0.237), ("24f", 3): (0.138, 0.209), ("24f", 16): (0.134, 0.209)}
DRIVER_CASE, DRIVER_K, DRIVER_INNER, DRIVER_TOL, DRIVER_MAXIT = "32v", 3, 5, 1e-8, 10
DRIVER_STEPS = {False: 11, True: 11}          # single -> inner steps of the oracle

_params, _runs = {}, {}


def param(mg, name, single=False, relaxType="VankaFaces", cycle=None, maxIter=5, tol=1e-30, flagged=True):
    """The case's hierarchy through MGsetup with ``vankaBlocks=flagged`` (cached: the device handle stays with it)."""
    n, levels, omega, cyc = CV.CASES[name]
    cyc = cycle or cyc
    key = (name, single, relaxType, cyc, maxIter, tol, flagged)
    if key not in _params:
        p = mg.getMGparam(np.complex128, np.int64, levels, 1, maxIter, tol, relaxType, CV.W, 1, 1, cyc, "NoMUMPS", 0.4, 0.0,
                          "SystemsFacesMixedLinear", singlePrecision=single, complexVanka=True, vankaBlocks=flagged)
        mg.MGsetup(CV.operator(n, omega), CV.mesh(mg, n), p)
        assert p.levels == levels
        _params[key] = p
    return _params[key]


def block(N, k, seed=5, zero_col=None, cx=True):
    """N x k Fortran-ordered block of seeded columns (column 0 is complex_vanka_cases.rhs for seed 5); zero_col: that column is 0."""
    B = np.asfortranarray(np.stack([V.seeded(N, seed + 7 * j, cx=cx) for j in range(k)], axis=1))
    if zero_col is not None:
        B[:, zero_col] = 0.0
    return B


def restate_block_relax(A, X, B, D, numit, n, ip, vtype):
    """``vanka_cases.restate_relax`` on every column; returns a new block."""
    out = np.array(X, order="F")
    for j in range(B.shape[1]):
        out[:, j] = V.restate_relax(A, np.array(X[:, j]), np.array(B[:, j]), D, numit, n, ip, vtype)
    return out


def restate_block_cycle(H, B, X, x_zero, cycle):
    """``complex_vanka_cases.restate_cycle`` on every column; x_zero is a property of the whole block.  Returns a new block."""
    out = np.zeros(B.shape, dtype=B.dtype, order="F")
    for j in range(B.shape[1]):
        out[:, j] = CV.restate_cycle(H, np.array(B[:, j]), None if x_zero else np.array(X[:, j]), x_zero, cycle)
    return out


def restate_block_history(H, B, cycles, cycle, tol=0.0):
    """solveMG on a block from X = 0 (SolveFuncs.jl:14-36; the rule of complex_block_oracle.solveMG): Frobenius norms of the whole
    block, stop after the cycle whose res / res_init < tol.  ([X after each cycle], [||R_0||, ||R_1||, ...])."""
    X = np.zeros(B.shape, dtype=B.dtype, order="F")
    Xs, res = [], [np.linalg.norm(B)]
    for it in range(cycles):
        X = restate_block_cycle(H, B, X, it == 0, cycle)
        Xs.append(X.copy())
        res.append(np.linalg.norm(B - H.As[0] @ X))
        if res[-1] / res[0] < tol:
            break
    return Xs, np.array(res)


def reference(mg, cid, k, cycles=2, zero_col=1):
    """(param, Hier, B, [X after each cycle], residual history) of a block case's complex128 restatement, computed once per
    (case, k, cycles) and left unchanged."""
    key = (cid, k, cycles, zero_col)
    if key not in _runs:
        name, kw = BLOCK_CYCLES[cid]
        p = param(mg, name, **kw)
        H = CV.Hier(p)
        B = block(p.As[0].shape[0], k, zero_col=zero_col)
        Xs, res = restate_block_history(H, B, cycles, p.cycleType)
        for a in Xs + [res, B]:
            a.setflags(write=False)
        _runs[key] = (p, H, B, Xs, res)
    return _runs[key]


def helmholtz_K(n, omega):
    """K = A_real - omega^2 (1 - 0.01i) S with S the 0/1 face selector (A_real - A_damped) / (omega^2 (1 - 0.1i))."""
    Ar = V.mixed_operator(n, True)
    Ad = CV.operator(n, omega)
    S = ((Ar - Ad) / (omega ** 2 * (1.0 - 0.1j))).tocsr()
    S = sp.csr_matrix(np.round(S.real))
    assert set(np.unique(S.diagonal())) == {0.0, 1.0} and (S - sp.diags(S.diagonal())).nnz == 0
    K = sp.csr_matrix(Ar.astype(np.complex128) - omega ** 2 * (1.0 - 0.01j) * S)
    K.sort_indices()
    return K


def driver_problem(mg, single):
    """(param, K, B) of the drivers' test: the flagged hierarchy of DRIVER_CASE with the drivers' tolerance, K and the k = 3 block."""
    n, _, omega, _ = CV.CASES[DRIVER_CASE]
    p = param(mg, DRIVER_CASE, single=single, maxIter=DRIVER_MAXIT, tol=DRIVER_TOL)
    K = helmholtz_K(n, omega)
    return p, K, block(K.shape[0], DRIVER_K)


def driver_oracle(mg, single):
    """blockFGMRES(DRIVER_INNER) of complex_block_fgmres_oracle on the drivers' problem with M = the column-wise restatement (the
    mixed closure for a ComplexF32 hierarchy): (X, flag, steps, resvec), computed once."""
    key = ("driver", single)
    if key not in _runs:
        p, K, B = driver_problem(mg, single)
        H = CV.Hier(p)
        if single:
            M1 = lambda v: CV.restate_cycle(H, v.astype(np.complex64), None, True, "V").astype(np.complex128)
        else:
            M1 = lambda v: CV.restate_cycle(H, v, None, True, "V")
        M = lambda Vb: np.stack([M1(np.array(Vb[:, j])) for j in range(Vb.shape[1])], axis=1)
        _runs[key] = bf.blockFGMRES(lambda Vb: K @ Vb, B, DRIVER_INNER, DRIVER_TOL, DRIVER_MAXIT, M)
    return _runs[key]
