"""TEST INFRASTRUCTURE ONLY.  numpy restatement of KrylovMethods.blockFGMRES as solveGMRES_MG calls it for size(b,2) > 1
(SolveFuncs.jl:130) with VAL = ComplexF64, the checker of mg_block_fgmres[_dev]_CFP64.  Imports no device code of the package.

This is ``blockFGMRES`` of oracle/mg_oracle.py (l.883-971: _chol_semidefinite, _tri_pinv_apply, _cholqr, blockFGMRES) for complex
blocks: Gram matrices are ``X.conj().T @ Y`` (H_ij = V_i^H W), the Cholesky factor of a Hermitian Gram matrix takes np.vdot for its
column products and the REAL diagonal for its pivots with the same ``rtol = 1e-14``, norms are Frobenius norms of moduli.  (The
oracle's own version casts its block to float64, so it cannot serve complex data; on real data the two agree,
tests/test_complex_block_fgmres_host.py pins that.)

The shared cases are those of tests/complex_krylov_oracle.py with the columns of tests/complex_block_oracle.py (``cb.block_rhs``)."""
from __future__ import annotations

import numpy as np


def _chol_semidefinite(G, rtol=1e-14):
    """Upper triangular Rf with G = Rf^H Rf for a Hermitian positive SEMI-definite Gram matrix; a column whose pivot falls to
    rtol * G[c,c] or below gets a zero row (its direction is dropped)."""
    k = G.shape[0]
    Rf = np.zeros((k, k), dtype=np.complex128)
    for c in range(k):
        g = G[c, c].real
        d = g - np.vdot(Rf[:c, c], Rf[:c, c]).real
        if g <= 0.0 or d <= rtol * g:
            continue
        Rf[c, c] = np.sqrt(d)
        for j in range(c + 1, k):
            Rf[c, j] = (G[c, j] - np.vdot(Rf[:c, c], Rf[:c, j])) / Rf[c, c]
    return Rf


def _tri_pinv_apply(W, Rf):
    """Q = W Rf^+ for the upper triangular Rf of _chol_semidefinite (zero pivots give zero columns of Q)."""
    k = Rf.shape[0]
    Q = np.zeros_like(W)
    for c in range(k):
        if Rf[c, c] == 0.0:
            continue
        Q[:, c] = (W[:, c] - Q[:, :c] @ Rf[:c, c]) / Rf[c, c]
    return Q


def _cholqr(W, stats=None):
    G = W.conj().T @ W
    if stats is not None:
        stats.append(np.linalg.cond(G))
    R1 = _chol_semidefinite(G)
    Q = _tri_pinv_apply(W, R1)
    R2 = _chol_semidefinite(Q.conj().T @ Q)
    Q = _tri_pinv_apply(Q, R2)
    return Q, R2 @ R1


def blockFGMRES(Afun, B, restrt, tol=1e-2, maxIter=100, M=None, X=None, stats=None):
    """oracle/mg_oracle.py's blockFGMRES for complex blocks.  Returns (X, flag, total inner steps, resvec); flags 0 / -1 / -9.
    stats (a list): receives cond(W^H W) of every Cholesky QR."""
    B = np.asarray(B, dtype=np.complex128)
    n, k = B.shape
    bn = np.linalg.norm(B)
    if bn == 0:
        return np.zeros((n, k), dtype=np.complex128), -9, 0, np.zeros(0)
    X = np.zeros((n, k), dtype=np.complex128) if X is None else np.array(X, dtype=np.complex128)
    Mf = M if M is not None else (lambda V: V.copy())
    R = B - Afun(X)
    if np.linalg.norm(R) / bn < tol:
        return X, 0, 0, np.zeros(0)
    m = restrt
    resvec, flag, total = [], -1, 0
    for it in range(1, maxIter + 1):
        V = [None] * (m + 1)
        Z = [None] * m
        H = np.zeros(((m + 1) * k, m * k), dtype=np.complex128)
        V[0], Rf = _cholqr(R, stats)
        xi = np.zeros(((m + 1) * k, k), dtype=np.complex128)
        xi[:k] = Rf
        used, Y = 0, None
        for j in range(m):
            Z[j] = Mf(V[j].copy()).copy()
            W = Afun(Z[j]).copy()
            for i in range(j + 1):
                Hij = V[i].conj().T @ W
                H[i * k:(i + 1) * k, j * k:(j + 1) * k] = Hij
                W = W - V[i] @ Hij
            V[j + 1], Hn = _cholqr(W, stats)
            H[(j + 1) * k:(j + 2) * k, j * k:(j + 1) * k] = Hn
            Hb = H[:(j + 2) * k, :(j + 1) * k]
            Y = np.linalg.lstsq(Hb, xi[:(j + 2) * k], rcond=None)[0]
            err = np.linalg.norm(xi[:(j + 2) * k] - Hb @ Y) / bn
            resvec.append(err)
            total += 1
            used = j + 1
            if err <= tol:
                flag = 0
                break
        for j in range(used):
            X = X + Z[j] @ Y[j * k:(j + 1) * k]
        if flag == 0:
            break
        R = B - Afun(X)
        if np.linalg.norm(R) / bn <= tol:
            flag = 0
            break
    return X, flag, total, np.array(resvec)


# ---- the shared runs: (case, k, inner) -> the inner steps the oracle takes (tests/test_complex_block_fgmres_host.py asserts them
# against the run itself, with the guard that keeps a rounding difference on the device from moving the stopping step) -----------
BLOCK_FGMRES_RUNS = {("C3", 3, 10): 20, ("C1", 2, 5): 56, ("C1", 4, 10): 41, ("C3", 16, 5): 17, ("C3", 1, 5): 31}

_runs = {}


def reference(mg, name, k, inner, maxIter=None, x0=None, key=None, single=False, stats=None):
    """The oracle's block run of a case, computed once and shared - nothing in it may be modified: (X, flag, steps, resvec).
    key: a name for a variant (x0 / maxIter given); single: the mixed closure of a ComplexF32 hierarchy
    (tests/complex_single_oracle.py) as M, column by column."""
    import complex_block_oracle as cb
    import complex_krylov_oracle as ck
    kk = (name, k, inner, key, single)
    if kk not in _runs:
        if single:
            import complex_single_oracle as cs
            p, As, _ = cs.case(mg, name)
            M1 = cs.preconditioner(p)
            M = lambda V: np.stack([M1(V[:, j]) for j in range(V.shape[1])], axis=1)
        else:
            p, As, _ = ck.case(mg, name)
            M = cb.preconditioner(p)
        B = cb.block_rhs(As.shape[0], k)
        _runs[kk] = blockFGMRES(lambda V: As @ V, B, inner, ck.TOL, ck.MAXIT_FGMRES if maxIter is None else maxIter, M, x0, stats)
    return _runs[kk]
