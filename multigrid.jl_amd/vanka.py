"""The Vanka cell-block smoother behind the reference's interface (src/Multigrid/Vanka.jl): ``getVankaRelaxType``,
``getVankaBlockSize``, ``getVankaVariablesOfCell``, ``cellColor``, ``cellRBColor``, ``setupVankaFacesPreconditioner`` on the
host (``device=True``: built on the device by vanka_build_blocks), ``RelaxVankaFacesColor`` on the device (csrc/mg_vanka.hpp
through ``mg_vanka_*``); there is no CPU fallback.

The reference sets ``const parallel = false`` (Vanka.jl:10): what runs there is the Julia serial path of RelaxVankaFacesColor
(l.383-425), and that is what is mirrored - not the red-black C path of deps/src/Vanka.c.

Unknowns of a RegularMesh of ``n`` cells: x-faces ((n1+1) n2 [n3], n1 fastest), y-faces, [z-faces,] then prod(n) cell
pressures when ``includePressure``.  This package holds the CSR of the applied operator A where Julia holds the CSC of AT = A'.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import scipy.sparse as sp

from . import device as D
from .dd_indices import cs2loc
from .domain_decomposition import cellColor

FULL_VANKA_RB = 1
KACMARZ_VANKA = 2
ECON_VANKA_RB = 3
FULL_VANKA_LEX = 4
FULL_VANKA_ADD = 5

_TYPES = {"VankaFaces": FULL_VANKA_RB, "EconVankaFaces": ECON_VANKA_RB, "VankaFacesLex": FULL_VANKA_LEX,
          "VankaFacesAdd": FULL_VANKA_ADD}


def getVankaRelaxType(s: str):
    """(isVanka, VankaType) of a relaxType string (Vanka.jl:20-32)."""
    return (True, _TYPES[s]) if s in _TYPES else (False, 0)


def toSingle(VAL):
    VAL = np.dtype(VAL)
    if VAL == np.float64:
        return np.dtype(np.float32)
    if VAL == np.complex128:
        return np.dtype(np.complex64)
    return VAL


def cellRBColor(i) -> int:
    return int(sum(int(k) for k in i)) % 2 + 1


def getVankaBlockSize(n, includePressure: bool):
    """(blockSize, nf): 4 / 5 in 2-D, 6 / 7 in 3-D; nf = faces per direction (Vanka.jl:211-222)."""
    n = np.asarray(n, dtype=np.int64)
    if n.size == 2:
        nf = np.array([(n[0] + 1) * n[1], n[0] * (n[1] + 1)], dtype=np.int64)
        return (5 if includePressure else 4), nf
    if n.size == 3:
        nf = np.array([(n[0] + 1) * n[1] * n[2], n[0] * (n[1] + 1) * n[2], n[0] * n[1] * (n[2] + 1)], dtype=np.int64)
        return (7 if includePressure else 6), nf
    raise ValueError("the face smoother serves 2-D and 3-D meshes")


def getVankaVariablesOfCell(i, n, nf, Idxs, includePressure: bool):
    """The (1-based, ascending) unknowns of the cell with 1-based per-dimension index ``i`` into Idxs (Vanka.jl:45-95)."""
    i = [int(k) for k in i]
    n = [int(k) for k in n]
    nf = [int(k) for k in nf]
    if len(i) == 2:
        t1 = i[0] + (i[1] - 1) * (n[0] + 1)
        t2 = nf[0] + i[0] + (i[1] - 1) * n[0]
        Idxs[0] = t1
        Idxs[1] = t1 + 1
        Idxs[2] = t2
        Idxs[3] = t2 + n[0]
        if includePressure:
            Idxs[4] = nf[1] + t2
        return Idxs
    t1 = i[0] + (n[0] + 1) * ((i[1] - 1) + n[1] * (i[2] - 1))
    t2 = nf[0] + i[0] + n[0] * ((i[1] - 1) + (n[1] + 1) * (i[2] - 1))
    t3 = nf[0] + nf[1] + i[0] + n[0] * ((i[1] - 1) + n[1] * (i[2] - 1))
    Idxs[0] = t1
    Idxs[1] = t1 + 1
    Idxs[2] = t2
    Idxs[3] = t2 + n[0]
    Idxs[4] = t3
    Idxs[5] = t3 + n[0] * n[1]
    if includePressure:
        Idxs[6] = nf[2] + t3
    return Idxs


def _mesh_n(M):
    return np.asarray(getattr(M, "n", M), dtype=np.int64)


def _weights(w, blockSize, includePressure):
    """(W, scalar?) of setupVankaFacesPreconditioner (Vanka.jl:305-313)."""
    if isinstance(w, (tuple, list, np.ndarray)):
        if len(w) != 2:
            raise ValueError("w is a Float64 or a tuple of two")
        W = np.full(blockSize, float(w[0]))
        if includePressure:
            W[-1] = float(w[1])
        return W, False
    return np.full(blockSize, float(w)), True


def _w_pair(w):
    """w as the C ABI takes it: (float64 array of 1 or 2 values, nw)."""
    if isinstance(w, (tuple, list, np.ndarray)):
        if len(w) != 2:
            raise ValueError("w is a Float64 or a tuple of two")
        return np.array([float(w[0]), float(w[1])], dtype=np.float64), 2
    return np.array([float(w)], dtype=np.float64), 1


def _check_build(lib, rc, what):
    """_check of a device build: a singular cell (MG_ERR_INVALID naming it) is numpy's LinAlgError, as np.linalg.inv raises it."""
    if rc == 1:
        msg = lib.mg_last_error()
        msg = msg.decode() if msg else ""
        if "singular" in msg:
            raise np.linalg.LinAlgError(f"{what}: {msg}")
    D._check(lib, rc, what)


def _setup_blocks_device(AT, M, w, includePressure, VankaType):
    """setupVankaFacesPreconditioner on the device: upload the operator, build (vanka_build_blocks), read back, close."""
    A = sp.csr_matrix(AT)
    if VankaType == KACMARZ_VANKA:
        raise NotImplementedError("KACMARZ_VANKA belongs to the hybrid cell-wise path (RelaxHybridVanka), which is out of scope")
    if VankaType not in (FULL_VANKA_RB, FULL_VANKA_LEX, ECON_VANKA_RB, FULL_VANKA_ADD):
        raise ValueError("unknown Vanka Type.")
    if VankaType == FULL_VANKA_LEX:
        raise NotImplementedError("FULL_VANKA_LEX is not served on the device (device=False sets its blocks up on the host)")
    if VankaType == ECON_VANKA_RB and isinstance(w, (tuple, list, np.ndarray)):
        raise TypeError("ECON_VANKA_RB takes a scalar w (Vanka.jl:361 divides the diagonal by it)")
    n = _mesh_n(M)
    blockSize, nf = getVankaBlockSize(n, includePressure)
    N = int(nf.sum()) + (int(np.prod(n)) if includePressure else 0)
    if A.shape != (N, N):
        raise ValueError(f"the operator is {A.shape}, a mesh of {n.tolist()} cells has {N} unknowns")
    with VankaHandle(A, None, n, includePressure, w=w, VankaType=VankaType) as H:
        return H.blocks()


def setupVankaFacesPreconditioner(AT, M, w, includePressure: bool, VankaType: int = FULL_VANKA_RB, device: bool = False):
    """LocalBlocks (Vanka.jl:294-370): per cell the adjoint of the damped inverse of Acc = A[I, I], in single precision,
    flattened column-major into column ``cell`` of a (bs^2, prod(n)) array.

    FULL_VANKA_RB / _LEX with a scalar w replace the leading (bs-1)x(bs-1) part of Acc by its diagonal (l.333: the line the
    reference runs IS the economic variant), a tuple w leaves Acc alone and scales the rows of its inverse; ECON_VANKA_RB
    divides that diagonal by w and does not damp further; FULL_VANKA_ADD halves the rows of faces shared with a neighbour.

    ``device=True`` (not in the reference's signature; default False: the host path below, untouched): the blocks are built on the
    device from the uploaded operator (mg_vanka_create_built_*) and read back - the same shape, dtype and memory order, the
    values those of the host path to the rounding of two double-precision eliminations; a singular cell raises
    ``np.linalg.LinAlgError``.  A complex64 operator is widened first, as the host path reads it."""
    if device:
        return _setup_blocks_device(AT, M, w, includePressure, VankaType)
    A = sp.csr_matrix(AT)
    n = _mesh_n(M)
    cx = np.iscomplexobj(A.data)
    blockSize, nf = getVankaBlockSize(n, includePressure)
    if VankaType == KACMARZ_VANKA:
        raise NotImplementedError("KACMARZ_VANKA belongs to the hybrid cell-wise path (RelaxHybridVanka), which is out of scope")
    if VankaType not in (FULL_VANKA_RB, FULL_VANKA_LEX, ECON_VANKA_RB, FULL_VANKA_ADD):
        raise ValueError("unknown Vanka Type.")
    N = int(nf.sum()) + (int(np.prod(n)) if includePressure else 0)
    if A.shape != (N, N):
        raise ValueError(f"the operator is {A.shape}, a mesh of {n.tolist()} cells has {N} unknowns")
    W, scalar = _weights(w, blockSize, includePressure)
    cells = int(np.prod(n))
    # every cell's index list at once (0-based); Acc[c] = A[I_c, I_c] by one sorted-key lookup per entry of the block
    I = _all_cell_indices(n, nf, includePressure) - 1
    loc = np.empty((cells, n.size), dtype=np.int64)
    c = np.arange(cells, dtype=np.int64)
    for d in range(n.size):
        loc[:, d] = c % n[d] + 1
        c = c // n[d]
    if not A.has_sorted_indices:
        A = A.copy()
        A.sort_indices()
    keys = np.repeat(np.arange(N, dtype=np.int64), np.diff(A.indptr)) * N + A.indices
    Acc = np.zeros((cells, blockSize, blockSize), dtype=np.complex128 if cx else np.float64)
    for t in range(blockSize):
        for j in range(blockSize):
            want = I[:, t] * N + I[:, j]
            pos = np.minimum(np.searchsorted(keys, want), max(keys.size - 1, 0))
            hit = keys[pos] == want
            Acc[hit, t, j] = A.data[pos[hit]]
    lead = np.arange(blockSize - 1)
    if VankaType in (FULL_VANKA_RB, FULL_VANKA_LEX):
        if scalar:
            dg = Acc[:, lead, lead].copy()
            Acc[:, :blockSize - 1, :blockSize - 1] = 0.0
            Acc[:, lead, lead] = dg
            Minv = float(w) * np.linalg.inv(Acc)
        else:
            Minv = W[None, :, None] * np.linalg.inv(Acc)
    elif VankaType == ECON_VANKA_RB:
        if not scalar:
            raise TypeError("ECON_VANKA_RB takes a scalar w (Vanka.jl:361 divides the diagonal by it)")
        dg = Acc[:, lead, lead] / float(w)
        Acc[:, :blockSize - 1, :blockSize - 1] = 0.0
        Acc[:, lead, lead] = dg
        Minv = np.linalg.inv(Acc)
    else:   # FULL_VANKA_ADD
        t = np.full((cells, blockSize), 0.5)
        for d in range(n.size):
            t[loc[:, d] == 1, 2 * d] = 1.0
            t[loc[:, d] == n[d], 2 * d + 1] = 1.0
        if includePressure:
            t[:, -1] = 1.0
        Minv = (t * W[None, :])[:, :, None] * np.linalg.inv(Acc)
    # AccInv = (..)' ; LocalBlocks[:, ii] = AccInv[:] (column-major): entry j + t*bs of a column is AccInv[j, t] = conj(Minv[t, j])
    blocks = np.conj(Minv).reshape(cells, blockSize * blockSize)
    return np.asfortranarray(blocks.T.astype(toSingle(Acc.dtype)))


def _all_cell_indices(n, nf, includePressure):
    """getVankaVariablesOfCell of every cell in linear order: (prod(n), blockSize), 1-based."""
    n = np.asarray(n, dtype=np.int64)
    cells = int(np.prod(n))
    bs, _ = getVankaBlockSize(n, includePressure)
    c = np.arange(cells, dtype=np.int64)
    i = []
    for d in range(n.size):
        i.append(c % n[d] + 1)
        c = c // n[d]
    out = np.empty((cells, bs), dtype=np.int64)
    if n.size == 2:
        t1 = i[0] + (i[1] - 1) * (n[0] + 1)
        t2 = nf[0] + i[0] + (i[1] - 1) * n[0]
        out[:, 0], out[:, 1], out[:, 2], out[:, 3] = t1, t1 + 1, t2, t2 + n[0]
        if includePressure:
            out[:, 4] = nf[1] + t2
        return out
    t1 = i[0] + (n[0] + 1) * ((i[1] - 1) + n[1] * (i[2] - 1))
    t2 = nf[0] + i[0] + n[0] * ((i[1] - 1) + (n[1] + 1) * (i[2] - 1))
    t3 = nf[0] + nf[1] + i[0] + n[0] * ((i[1] - 1) + n[1] * (i[2] - 1))
    out[:, 0], out[:, 1], out[:, 2], out[:, 3], out[:, 4], out[:, 5] = t1, t1 + 1, t2, t2 + n[0], t3, t3 + n[0] * n[1]
    if includePressure:
        out[:, 6] = nf[2] + t3
    return out


# ---- the device relaxation --------------------------------------------------------------------------------------------
_fp = C.POINTER(C.c_float)


class VankaHandle:
    """An uploaded (operator, blocks, mesh) triple: one mg_vanka handle, owned by whoever holds this object.  A caller that
    relaxes with the same operator many times builds it once (``vanka_handle``) and passes it to ``RelaxVankaFacesColor``;
    after changing the operator's or the blocks' values it closes it and builds another - nothing is cached behind its back."""

    def __init__(self, A, Dblk, n, includePressure, w=None, VankaType: int = FULL_VANKA_RB):
        """``Dblk``: the cells' blocks, or None with ``w`` (a float or a pair): the blocks are built on the device from the
        uploaded operator for (w, VankaType) (mg_vanka_create_built_*)."""
        A = A if sp.isspmatrix_csr(A) and A.has_sorted_indices else _sorted_csr(A)
        lib = D.load_library()
        self.cx = bool(np.iscomplexobj(A.data))
        self.N = int(A.shape[0])
        self.n = tuple(int(k) for k in n)
        self.includePressure = bool(includePressure)
        self.nnz = int(A.nnz)
        cp = np.ascontiguousarray(A.indptr, dtype=np.int64) + 1
        rv = np.ascontiguousarray(A.indices, dtype=np.int64) + 1
        nz = np.ascontiguousarray(A.data, dtype=np.complex128 if self.cx else np.float64)
        nn = np.ascontiguousarray(n, dtype=np.int64)
        self.h = C.c_void_p()
        sfx = "CFP64_INT64" if self.cx else "FP64_INT64"
        if Dblk is None:
            if w is None:
                raise ValueError("a Vanka handle takes the cells' blocks, or w (and VankaType) to build them on the device")
            wv, nw = _w_pair(w)
            _check_build(lib, getattr(lib, f"mg_vanka_create_built_{sfx}")(0, nn.size, D._i64(nn), 1 if includePressure else 0, A.shape[0],
                                                                            D._i64(cp), D._i64(rv), D._f64(nz), int(VankaType), D._f64(wv), nw,
                                                                            C.byref(self.h)), "mg_vanka_create_built")
            return
        blk = np.asfortranarray(Dblk, dtype=np.complex64 if self.cx else np.float32)
        D._check(lib, getattr(lib, f"mg_vanka_create_{sfx}")(0, nn.size, D._i64(nn), 1 if includePressure else 0, A.shape[0], D._i64(cp),
                                                             D._i64(rv), D._f64(nz), blk.ctypes.data_as(_fp), C.byref(self.h)), "mg_vanka_create")

    def info(self):
        return vanka_info(self.h)

    def build_blocks(self, w, VankaType: int = FULL_VANKA_RB):
        """The handle's blocks again from its resident operator (mg_vanka_build_blocks_*): ``w`` a float or a pair.  A singular
        cell raises ``np.linalg.LinAlgError`` and the handle keeps the blocks it had."""
        lib = D.load_library()
        wv, nw = _w_pair(w)
        fn = lib.mg_vanka_build_blocks_CFP64 if self.cx else lib.mg_vanka_build_blocks_FP64
        _check_build(lib, fn(self.h, int(VankaType), D._f64(wv), nw), "mg_vanka_build_blocks")

    def replace_values(self, A):
        """New values of the operator on the uploaded pattern (mg_vanka_replace_values_*); the blocks stay until ``build_blocks``."""
        A = A if sp.isspmatrix_csr(A) and A.has_sorted_indices else _sorted_csr(A)
        if A.shape != (self.N, self.N) or A.nnz != self.nnz:
            raise ValueError("replace_values takes an operator of the uploaded pattern")
        if np.iscomplexobj(A.data) and not self.cx:
            raise TypeError("complex values for a handle of a real operator")
        lib = D.load_library()
        nz = np.ascontiguousarray(A.data, dtype=np.complex128 if self.cx else np.float64)
        fn = lib.mg_vanka_replace_values_CFP64 if self.cx else lib.mg_vanka_replace_values_FP64
        D._check(lib, fn(self.h, D._f64(nz), nz.size), "mg_vanka_replace_values")

    def blocks(self):
        """The handle's blocks as setupVankaFacesPreconditioner returns them: (bs^2, cells), float32 / complex64, column-major."""
        lib = D.load_library()
        bs = getVankaBlockSize(np.asarray(self.n), self.includePressure)[0]
        out = np.zeros((bs * bs, int(np.prod(self.n))), dtype=np.complex64 if self.cx else np.float32, order="F")
        D._check(lib, lib.mg_vanka_get_blocks(self.h, out.ctypes.data_as(_fp), out.size), "mg_vanka_get_blocks")
        return out

    def apply_dev(self, x, b, numit: int, VankaType: int = FULL_VANKA_RB):
        """``numit`` iterations on torch device tensors, x in place, waited for: 1-D vectors (mg_vanka_apply_dev_*) or contiguous
        row-major blocks [N, k], 1 <= k <= 16 (mg_vanka_apply_block_dev_*); float64 for a real handle, complex128 for a complex one."""
        import torch
        want = torch.complex128 if self.cx else torch.float64
        for t in (x, b):
            if not (hasattr(t, "dtype") and hasattr(t, "data_ptr")) or t.dtype != want:
                raise TypeError(f"expected {want} device tensors")
            if t.dim() not in (1, 2) or not t.is_contiguous() or t.shape[0] != self.N:
                raise ValueError(f"device vectors hold {self.N} values, device blocks are contiguous [{self.N}, k] tensors")
        if tuple(x.shape) != tuple(b.shape):
            raise ValueError("x and b must have the same shape")
        lib = D.load_library()
        D._sync_torch(x, b)
        sfx = "CFP64" if self.cx else "FP64"
        if x.dim() == 1:
            D._check(lib, getattr(lib, f"mg_vanka_apply_dev_{sfx}")(self.h, D._ptr(x), D._ptr(b), int(numit), int(VankaType)),
                     "mg_vanka_apply_dev")
        else:
            if not 1 <= int(x.shape[1]) <= D.BLOCK_KMAX:
                raise NotImplementedError(f"a Vanka block holds 1 to {D.BLOCK_KMAX} right-hand sides ({int(x.shape[1])} given)")
            D._check(lib, getattr(lib, f"mg_vanka_apply_block_dev_{sfx}")(self.h, D._ptr(x), D._ptr(b), int(x.shape[1]), int(numit),
                                                                         int(VankaType)), "mg_vanka_apply_block_dev")
        return x

    def close(self):
        if getattr(self, "h", None):
            D.load_library().mg_vanka_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def vanka_handle(A, Dblk, n, includePressure, w=None, VankaType: int = FULL_VANKA_RB) -> VankaHandle:
    """Upload operator and blocks once; the caller holds the handle and closes it.  ``Dblk=None`` with ``w`` (and ``VankaType``):
    the blocks are built on the device from the uploaded operator."""
    return VankaHandle(A, Dblk, _mesh_n(n), includePressure, w=w, VankaType=VankaType)


def _sorted_csr(A):
    A = sp.csr_matrix(A).copy()
    A.sort_indices()
    return A


def vanka_info(h):
    info = (C.c_longlong * 8)()
    lib = D.load_library()
    D._check(lib, lib.mg_vanka_info(h, info), "mg_vanka_info")
    return [int(v) for v in info]


def RelaxVankaFacesColor(AT, x, b, Dblk, numit: int, numCores: int, M, includePressure: bool, VankaType: int = FULL_VANKA_RB,
                         handle: "VankaHandle | None" = None):
    """``numit`` Vanka iterations of x towards A x = b, in place, on the device (Vanka.jl:372-434); returns x.

    The reference hands AT.nzval and D over on every call, and so does this: operator and blocks are uploaded for the call and
    released after it.  ``handle`` (not in the reference's signature): a ``vanka_handle`` the caller built from this operator,
    these blocks and this mesh - then nothing is uploaded.

    FULL_VANKA_RB / ECON_VANKA_RB: per iteration 2^dim coloured passes, each from a snapshot of x.  FULL_VANKA_ADD: the
    corrections are formed once per call from the incoming x and added numit times (l.396-405).  numit = 0 does nothing.

    A 2-D ``x`` and ``b`` (N x k, 1 <= k <= 16, not in the reference) are relaxed as a block by one pass over the operator and the
    blocks (mg_vanka_apply_block_*): column c gets the bits of the call on column c alone."""
    x_arr = np.asarray(x)
    b_arr = np.asarray(b)
    cx = np.iscomplexobj(AT.data if sp.issparse(AT) else AT)
    for name, a in (("x", x_arr), ("b", b_arr)):
        if a.dtype.kind == "c" and not cx:
            raise TypeError(f"RelaxVankaFacesColor: {name} is {a.dtype} but the operator is real")
        if a.dtype != (np.complex128 if cx else np.float64):
            raise TypeError(f"RelaxVankaFacesColor: {name} is {a.dtype}, expected {'complex128' if cx else 'float64'}")
    if not isinstance(Dblk, np.ndarray) or Dblk.dtype != toSingle(x_arr.dtype):
        raise TypeError("check types.")     # (Vanka.jl:375-377)
    if VankaType == FULL_VANKA_LEX:
        raise NotImplementedError("FULL_VANKA_LEX is a sequential sweep over the cells; the package keeps no CPU fallback")
    if VankaType == KACMARZ_VANKA:
        raise NotImplementedError("KACMARZ_VANKA belongs to the hybrid cell-wise path (RelaxHybridVanka), which is out of scope")
    if VankaType not in (FULL_VANKA_RB, ECON_VANKA_RB, FULL_VANKA_ADD):
        raise ValueError("unknown Vanka Type.")
    n = _mesh_n(M)
    blockSize, nf = getVankaBlockSize(n, includePressure)
    N = int(nf.sum()) + (int(np.prod(n)) if includePressure else 0)
    block = x_arr.ndim == 2 and b_arr.ndim == 2
    if block:
        if x_arr.shape != b_arr.shape or x_arr.shape[0] != N:
            raise ValueError(f"blocks x and b must both be {N} x k for a mesh of {n.tolist()} cells")
        if not 1 <= x_arr.shape[1] <= D.BLOCK_KMAX:
            raise NotImplementedError(f"a Vanka block holds 1 to {D.BLOCK_KMAX} right-hand sides ({x_arr.shape[1]} given)")
    elif x_arr.ndim != 1 or b_arr.ndim != 1 or x_arr.shape[0] != N or b_arr.shape[0] != N:
        raise ValueError(f"x and b must be vectors of sum(nf) [+ prod(n)] = {N} values for a mesh of {n.tolist()} cells")
    if Dblk.shape != (blockSize * blockSize, int(np.prod(n))):
        raise ValueError(f"D must be {(blockSize * blockSize, int(np.prod(n)))}, got {Dblk.shape}")
    if AT.shape != (N, N):
        raise ValueError(f"the operator is {AT.shape}, expected {(N, N)}")
    if not (isinstance(x, np.ndarray) and (x.flags.c_contiguous or (block and x.flags.f_contiguous)) and x.flags.writeable):
        raise ValueError("x must be a contiguous writable array (it is relaxed in place)")
    if int(numit) < 0:
        raise ValueError("numit must be >= 0")
    own = handle is None
    if not own and (handle.cx != cx or handle.N != N or handle.n != tuple(int(k) for k in n) or handle.includePressure != bool(includePressure)):
        raise ValueError("the handle was built for another operator, mesh or value type")
    H = VankaHandle(AT, Dblk, n, includePressure) if own else handle
    try:
        lib = D.load_library()
        if block:                       # the host entry takes column-major N x k
            xf = np.asfortranarray(x)
            bf = np.asfortranarray(b_arr)
            apply = lib.mg_vanka_apply_block_CFP64 if cx else lib.mg_vanka_apply_block_FP64
            D._check(lib, apply(H.h, D._f64(xf), D._f64(bf), int(x.shape[1]), int(numit), int(VankaType)), "mg_vanka_apply_block")
            if not np.shares_memory(xf, x):
                x[...] = xf
        else:
            bb = np.ascontiguousarray(b_arr)
            apply = lib.mg_vanka_apply_CFP64 if cx else lib.mg_vanka_apply_FP64
            D._check(lib, apply(H.h, D._f64(x), D._f64(bb), int(numit), int(VankaType)), "mg_vanka_apply")
    finally:
        if own:
            H.close()
    return x
