"""Transfer operators of staggered-grid systems (src/Multigrid/Systems.jl), in scipy, 2-D and 3-D.

``n`` is always in cells.  Unknowns: x-faces, y-faces [, z-faces] [, cell centres].  A face block of direction j is nodal in
dimension j and cell-centred in the others: its operators are Kronecker products of the five 1-D operators below, the last
dimension outermost (``kron(R3, kron(R2, R1))``).  Every 1-D operator is the identity below 8 cells - that is what stops the
coarsening in MGsetup (a square P).
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp


def _speye(n):
    return sp.identity(n, dtype=np.float64, format="csr")


def _even(n, who):
    nc = n // 2
    if 2 * nc != n:
        raise ValueError(f"Err: {who}(): size should be a multiplication of 2")
    return nc


def get1DNodeInjection(n_cells: int):
    """Node injection C,F,C,...,C: (nc+1) x (n+1) (Systems.jl:80-93)."""
    n = int(n_cells)
    if n < 8:
        return _speye(n + 1), n
    nc = _even(n, "get1DNodeInjection")
    return _speye(n + 1)[0:n + 1:2, :].tocsr(), nc


def get1DNodeFullWeightRestriction(n_cells: int):
    """Full weighting on nodes, doubled: rows (.5, 1, .5); the boundary rows are the cut-off columns of the tridiagonal
    matrix, (1, .5) and (.5, 1) (Systems.jl:95-111)."""
    n = int(n_cells)
    if n < 8:
        return _speye(n + 1), n
    nc = _even(n, "get1DNodeFullWeightRestriction")
    R = sp.diags([np.full(n, .25), np.full(n + 1, .5), np.full(n, .25)], [-1, 0, 1], shape=(n + 1, n + 1), format="csc")
    R = (R[:, 0:n + 1:2].T * 2.0).tocsr()
    return R, nc


def get1DProlongationCellCentered(ncells_fine: int):
    """[C, C] -> [F, F, F, F] with weights (1/4, 3/4): n x nc (Systems.jl:114-132).

    Julia's ``spdiagm(-2 => fill(.25, n-2), -1 => fill(.75, n-1), 0 => fill(.75, n-1), 1 => fill(.25, n-1))`` is n x n with
    only n-1 entries on the main diagonal: entry (n, n) stays zero.  Every second column is kept (1, 3, ... in Julia's
    count), then the two corners are overwritten: P[1, 1] = 1 and P[end, end] = 1."""
    n = int(ncells_fine)
    if n < 8:
        return _speye(n), n
    nc = _even(n, "get1DProlongationCellCentered")
    main = np.concatenate([np.full(n - 1, .75), [0.0]])
    P = sp.diags([np.full(n - 2, .25), np.full(n - 1, .75), main, np.full(n - 1, .25)], [-2, -1, 0, 1], shape=(n, n), format="csc")
    P = P[:, 0:n:2].tolil()
    P[0, 0] = 1.0
    P[n - 1, nc - 1] = 1.0
    P = P.tocsr()
    P.eliminate_zeros()
    return P, nc


def get1DRestrictionCells(n: int):
    """2 x 1 aggregation, doubled: rows (1, 1): nc x n (Systems.jl:134-148)."""
    n = int(n)
    if n < 8:
        return _speye(n), n
    nc = _even(n, "get1DRestrictionCells")
    R = sp.diags([np.full(n - 1, .5), np.full(n - 1, .5)], [0, 1], shape=(n - 1, n), format="csr")
    return (2.0 * R[0:n:2, :]).tocsr(), nc


def get1DProlongationNodes(ncells_fine: int):
    """Linear interpolation on nodes: (n+1) x (nc+1), columns (.5, 1, .5) (Systems.jl:150-164)."""
    n = int(ncells_fine)
    if n < 8:
        return _speye(n + 1), n
    nc = _even(n, "get1DProlongationNodes")
    P = sp.diags([np.full(n, .5), np.ones(n + 1), np.full(n, .5)], [-1, 0, 1], shape=(n + 1, n + 1), format="csc")
    return P[:, 0:n + 1:2].tocsr(), nc


def _kron_all(ops):
    """kron(ops[dim-1], ... kron(ops[1], ops[0])): the first dimension runs fastest."""
    if len(ops) not in (2, 3):
        raise ValueError("Dimension not supported!")
    K = ops[0]
    for M in ops[1:]:
        K = sp.kron(M, K, format="csr")
    K = sp.csr_matrix(K)
    K.sort_indices()
    return K


def _per_dim(n, j, nodal, cells):
    n = [int(k) for k in np.asarray(n).ravel()]
    ops, nc = [], []
    for kk in range(len(n)):
        M, c = (nodal if kk + 1 == j else cells)(n[kk])
        ops.append(M)
        nc.append(c)
    return _kron_all(ops), np.asarray(nc, dtype=np.int64)


def getRestrictionCellCentered(n):
    return _per_dim(n, 0, None, get1DRestrictionCells)


def getRestrictionFacesInjectionUj(n, j: int):
    return _per_dim(n, j, get1DNodeInjection, get1DRestrictionCells)


def getRestrictionFacesFullWeightUj(n, j: int):
    return _per_dim(n, j, get1DNodeFullWeightRestriction, get1DRestrictionCells)


def getLinearInterpolationFacesUj(n, j: int):
    return _per_dim(n, j, get1DProlongationNodes, get1DProlongationCellCentered)


def getLinearInterpolationCellCentered(n):
    return _per_dim(n, 0, None, get1DProlongationCellCentered)


def _blockdiag(blocks):
    M = sp.block_diag(blocks, format="csr")
    M.sort_indices()
    return M


def getInjectionOperatorsSystemsFaces(n, withCellsBlock: bool):
    """blockdiag of the face injections [and the cell restriction] (Systems.jl:8-31)."""
    dim = len(np.asarray(n).ravel())
    R = [getRestrictionFacesInjectionUj(n, j)[0] for j in range(1, dim + 1)]
    if withCellsBlock:
        R.append(getRestrictionCellCentered(n)[0])
    return _blockdiag(R)


def getLinearOperatorsSystemsFaces(n, withCellsBlock: bool):
    """(P, R, nc): linear interpolation and full weighting per face block [, and the cell-centred pair] (Systems.jl:33-76)."""
    dim = len(np.asarray(n).ravel())
    P, R, nc = [], [], None
    for j in range(1, dim + 1):
        Pj, ncj = getLinearInterpolationFacesUj(n, j)
        if nc is None:
            nc = ncj
        P.append(Pj)
        R.append(getRestrictionFacesFullWeightUj(n, j)[0])
    if withCellsBlock:
        P.append(getLinearInterpolationCellCentered(n)[0])
        R.append(getRestrictionCellCentered(n)[0])
    return _blockdiag(P), _blockdiag(R), nc
