"""Shared by the tests of the device set-up of the Vanka blocks (vanka_build_blocks, csrc/mg_vanka.hpp): the cases, a numpy
restatement of the kernel's elimination, and the tolerance of a block comparison.  Imports no device code of the package.

The restatement does per cell what one eight-lane group does: gather Acc = A[I, I] from the sorted rows (an absent entry is zero),
apply the variant's edit, run Gauss-Jordan with partial pivoting on [Acc | I] - the pivot of column k is the entry of largest
squared modulus among rows k .. bs-1, the lowest row on ties; rows k and the pivot's change places; the pivot row is multiplied by
the pivot's reciprocal and taken out of every other row - scale row t of the inverse, conjugate, cast to single, and lay the block
out as LocalBlocks (entry j + t*bs of column `cell`).  All in double.  It is vectorised over the cells.

Tolerance of a block comparison, per real or imaginary component:  |dev - host| <= spacing32(|host|) + 2^-40 * max|host block|.
Both sides invert in double; the full cell blocks of these operators have a condition number of at most 8.8 (measured on [6,5,4],
omega = 0.15), so their double-precision error is below 2^-45 of the block's norm: the second term leaves a factor 32 over that,
the first is one rounding step to single."""
import numpy as np
import scipy.sparse as sp

import vanka_cases as V

OMEGA, MASS = 0.15, 1e-2        # the complex operators: complex_vanka_cases.operator's damping and mass
W_SCALAR, W_PAIR = 0.6, (0.6, 0.4)
# (VankaType, w): types 1, 3 and 5, the scalar and the pair (type 3 takes a scalar only)
VARIANTS = [(V.FULL_VANKA_RB, W_SCALAR), (V.FULL_VANKA_RB, W_PAIR), (V.ECON_VANKA_RB, W_SCALAR), (V.FULL_VANKA_ADD, W_SCALAR),
            (V.FULL_VANKA_ADD, W_PAIR)]
# (cells, includePressure): n = 1 in a direction, 30 cells (a partial workgroup of 32 groups), 360 cells (several workgroups)
MESHES = [([3, 2], True), ([3, 2], False), ([1, 4], True), ([1, 4], False), ([3, 2, 2], True), ([5, 3, 2], True), ([9, 8, 5], True),
          ([4, 1, 3], False)]

_ops = {}


def operator(n, ip, cx):
    """The mixed operator of vanka_cases (complex: complex_vanka_cases.operator's omega and mass)."""
    key = (tuple(n), bool(ip), bool(cx))
    if key not in _ops:
        _ops[key] = V.mixed_operator(n, ip, omega=OMEGA if cx else None, mass=MASS)
    return _ops[key]


def thinned(A, seed=7):
    """A with about a third of its off-diagonal entries taken out of the PATTERN (seeded; the diagonal stays)."""
    C = sp.coo_matrix(A)
    rng = np.random.default_rng(seed)
    keep = (C.row == C.col) | (rng.random(C.nnz) >= 1.0 / 3.0)
    T = sp.csr_matrix((C.data[keep], (C.row[keep], C.col[keep])), shape=A.shape)
    T.sort_indices()
    return T


def zero_row_of_cell(A, n, ip, cell=1, slot=0):
    """A (same pattern) with the row of unknown `slot` of 0-based `cell` zeroed: that cell's block is singular."""
    I = V.all_unknowns(n, ip) - 1
    B = sp.csr_matrix(A, copy=True)
    r = int(I[cell, slot])
    B.data[B.indptr[r]:B.indptr[r + 1]] = 0.0
    return B


def gather(A, n, ip):
    """Acc[c] = A[I_c, I_c] densely, (cells, bs, bs) in double / complex double."""
    A = sp.csr_matrix(A)
    I = V.all_unknowns(n, ip) - 1
    cells, bs = I.shape
    Acc = np.zeros((cells, bs, bs), dtype=np.complex128 if np.iscomplexobj(A.data) else np.float64)
    for c in range(cells):
        Acc[c] = A[I[c], :][:, I[c]].toarray()
    return Acc


def gauss_jordan(Acc):
    """inv(Acc[c]) for every c by the kernel's elimination; raises np.linalg.LinAlgError at a zero or non-finite pivot."""
    cells, bs, _ = Acc.shape
    cx = np.iscomplexobj(Acc)
    M = np.concatenate([Acc, np.broadcast_to(np.eye(bs, dtype=Acc.dtype), Acc.shape)], axis=2).copy()
    c = np.arange(cells)
    for k in range(bs):
        col = M[:, k:, k]
        m2 = col.real ** 2 + col.imag ** 2 if cx else col * col
        at = k + np.argmax(m2, axis=1)                       # (argmax: the first of equal maxima = the lowest row)
        best = m2[c, at - k]
        if not np.all((best > 0.0) & np.isfinite(best)):
            raise np.linalg.LinAlgError("Singular matrix")
        rk, ra = M[c, k, :].copy(), M[c, at, :].copy()
        M[c, at, :] = rk
        p = ra[:, k]
        rp = (p.real / best - 1j * (p.imag / best)) if cx else 1.0 / p
        pr = rp[:, None] * ra
        f = M[:, :, k].copy()
        f[:, k] = 0.0
        M -= f[:, :, None] * pr[:, None, :]
        M[:, k, :] = pr
    return M[:, :, bs:]


def restate_blocks(A, n, w, ip, vtype):
    """LocalBlocks as the kernel builds them: (bs^2, cells) float32 / complex64, column-major."""
    n = [int(k) for k in n]
    Acc = gather(A, n, ip)
    cells, bs, _ = Acc.shape
    pair = isinstance(w, (tuple, list))
    W = np.full(bs, float(w[0]) if pair else float(w))
    if pair and ip:
        W[-1] = float(w[1])
    if vtype == V.ECON_VANKA_RB and pair:
        raise TypeError("ECON_VANKA_RB takes a scalar w")
    if not pair and vtype in (V.FULL_VANKA_RB, V.ECON_VANKA_RB):
        lead = np.arange(bs - 1)
        dg = Acc[:, lead, lead].copy()
        if vtype == V.ECON_VANKA_RB:
            dg = dg / float(w)
        Acc[:, :bs - 1, :bs - 1] = 0.0
        Acc[:, lead, lead] = dg
    Minv = gauss_jordan(Acc)
    if vtype == V.FULL_VANKA_RB:
        s = np.broadcast_to(W, (cells, bs))
    elif vtype == V.ECON_VANKA_RB:
        s = np.ones((cells, bs))
    else:
        t = np.full((cells, bs), 0.5)
        for ii in range(cells):
            loc = V.cs2loc(ii + 1, n)
            for d in range(len(n)):
                if loc[d] == 1:
                    t[ii, 2 * d] = 1.0
                if loc[d] == n[d]:
                    t[ii, 2 * d + 1] = 1.0
        if ip:
            t[:, -1] = 1.0
        s = t * W[None, :]
    Minv = s[:, :, None] * Minv
    single = np.complex64 if np.iscomplexobj(Minv) else np.float32
    return np.asfortranarray(np.conj(Minv).reshape(cells, bs * bs).T.astype(single))


def block_excess(dev, host):
    """(largest |dev - host| over its bound, share of components whose bits differ): the comparison passes where the first is <= 1."""
    assert dev.shape == host.shape and dev.dtype == host.dtype
    scale = np.abs(host).max(axis=0, keepdims=True).astype(np.float64)            # max |entry| of each cell's block
    worst, differ, count = 0.0, 0, 0
    parts = [(dev.real, host.real), (dev.imag, host.imag)] if np.iscomplexobj(host) else [(dev, host)]
    for d, h in parts:
        bound = np.spacing(np.abs(h)).astype(np.float64) + 2.0 ** -40 * scale
        worst = max(worst, float((np.abs(d.astype(np.float64) - h.astype(np.float64)) / bound).max()))
        differ += int(np.count_nonzero(d.view(np.uint32) != h.view(np.uint32)))
        count += h.size
    return worst, differ / count
