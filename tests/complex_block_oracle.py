"""TEST INFRASTRUCTURE ONLY.  numpy restatement of what the reference does with a BLOCK of right-hand sides for VAL = ComplexF64,
the checker of the mg_block_* entry points.  Imports no device code of the package.

  * One cycle on a block (getMultigridPreconditioner, SolveFuncs.jl:43-63): the cycle is column-separable - every product, update and
    coarsest solve acts on the columns independently - so it is tests/complex_oracle.py's recursiveCycle column by column.  The one
    thing the block decides as a whole is ``norm(x) > 0`` (MGcycle.jl:29); for a column that is zero inside a non-zero block the
    residual branch computes b - A*0 = b, the value the other branch takes.
  * solveMG on a block (SolveFuncs.jl:14-36): the same loop with Frobenius norms of the whole block.
  * KrylovMethods.blockBiCGSTB as solveBiCGSTAB_MG calls it for size(b,2) > 1 (SolveFuncs.jl:94-96): ``blockBiCGSTB`` of
    oracle/mg_oracle.py with complex blocks - Gram matrices R0^H V, R0^H R, omega = tr(T^H S) / tr(T^H T) by np.vdot, column norms of
    moduli.  (The oracle's own version casts its block to float64, so it cannot serve complex data; on real data the two agree,
    tests/test_complex_block_host.py pins that.)"""
from __future__ import annotations

import numpy as np

import complex_oracle as corc


def block_cycle(param, B, X):
    """X[:, j] <- recursiveCycle(param, B[:, j], X[:, j], 1) for every column; X updated in place and returned."""
    mem = corc._Mem(param)
    for j in range(B.shape[1]):
        xj = np.array(X[:, j], dtype=np.complex128)
        X[:, j] = corc.recursiveCycle(param, np.array(B[:, j], dtype=np.complex128), xj, 1, mem)
    return X


def preconditioner(param):
    """M(V) = one cycle from zero on every column (SolveFuncs.jl:59 on a block)."""

    def M(V):
        return block_cycle(param, V, np.zeros(V.shape, dtype=np.complex128))

    return M


def solveMG(param, B, X, history=None):
    """SolveFuncs.jl:3-39 on a block: norms are Frobenius norms.  X updated in place; returns (X, iter)."""
    A = param.As[0]
    res_init = np.linalg.norm(B) if np.linalg.norm(X) == 0 else np.linalg.norm(B - A @ X)
    resvec = [res_init]
    it = 0
    for _ in range(param.maxOuterIter):
        block_cycle(param, B, X)
        it += 1
        res = np.linalg.norm(B - A @ X)
        resvec.append(res)
        if res / res_init < param.relativeTol:
            break
    if isinstance(history, dict):
        history["resvec"] = np.array(resvec)
    return X, it


def _colnorms(V):
    return np.sqrt((np.abs(V) ** 2).sum(axis=0))


def blockBiCGSTB(Afun, B, tol=1e-6, maxIter=100, M1=None, X=None):
    """oracle/mg_oracle.py's blockBiCGSTB for complex blocks.  Returns (X, flag, iterations, resvec); flags 0 / -1 / -2 / -3 / -9."""
    B = np.asarray(B, dtype=np.complex128)
    n, k = B.shape
    nb = _colnorms(B)
    if not np.any(nb > 0):
        return np.zeros((n, k), dtype=np.complex128), -9, 0, np.zeros(0)
    nb = np.where(nb > 0, nb, 1.0)
    X = np.zeros((n, k), dtype=np.complex128) if X is None else np.array(X, dtype=np.complex128)
    Mf = M1 if M1 is not None else (lambda V: V.copy())
    R = B - Afun(X)
    resvec = [(_colnorms(R) / nb).max()]
    if resvec[0] < tol:
        return X, 0, 0, np.array(resvec)
    R0 = R.copy()
    P = R.copy()
    flag, it = -1, 0
    for it in range(1, maxIter + 1):
        Phat = Mf(P).copy()
        V = Afun(Phat).copy()
        RtV = R0.conj().T @ V
        alpha = np.linalg.solve(RtV, R0.conj().T @ R)
        S = R - V @ alpha
        sn = (_colnorms(S) / nb).max()
        resvec.append(sn)
        if sn < tol:
            X = X + Phat @ alpha
            flag = -3
            break
        Shat = Mf(S).copy()
        T = Afun(Shat).copy()
        tt = np.vdot(T, T).real
        if tt == 0.0:
            flag = -2
            break
        omega = np.vdot(T, S) / tt
        X = X + Phat @ alpha + omega * Shat
        R = S - omega * T
        err = (_colnorms(R) / nb).max()
        resvec.append(err)
        if err <= tol:
            flag = 0
            break
        if omega == 0.0:
            flag = -2
            break
        beta = -np.linalg.solve(RtV, R0.conj().T @ T)
        P = R + (P - omega * V) @ beta
    return X, flag, it, np.array(resvec)


# ---- the shared block cases: complex_krylov_oracle.CASES with the columns complex_rhs(n, 40 + j) ---------------------------------
# (case, k) -> what the oracle takes (asserted by tests/test_complex_block_host.py against the run itself): (iterations, flag)
BLOCK_RUNS = {("C3", 3): (11, -3), ("C1", 5): (17, 0), ("C1", 2): (19, 0)}

_runs = {}


def block_rhs(n, k):
    from complex_cases import complex_rhs
    return np.asfortranarray(np.stack([complex_rhs(n, 40 + j) for j in range(k)], axis=1))


def reference(mg, name, k, maxIter=None, key=None, single=False):
    """The oracle's block run of a case, computed once and shared: (X, flag, iterations, resvec).  single: the mixed closure of a
    ComplexF32 hierarchy (tests/complex_single_oracle.py) as M1, column by column."""
    import complex_krylov_oracle as ck
    kk = (name, k, key, single)
    if kk not in _runs:
        if single:
            import complex_single_oracle as cs
            p, As, _ = cs.case(mg, name)
            M1 = cs.preconditioner(p)
            M = lambda V: np.stack([M1(V[:, j]) for j in range(V.shape[1])], axis=1)
        else:
            p, As, _ = ck.case(mg, name)
            M = preconditioner(p)
        B = block_rhs(As.shape[0], k)
        _runs[kk] = blockBiCGSTB(lambda V: As @ V, B, ck.TOL, ck.MAXIT_BICGSTAB if maxIter is None else maxIter, M)
    return _runs[kk]
