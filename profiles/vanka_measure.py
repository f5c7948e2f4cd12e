"""One FULL_VANKA_RB iteration of the Vanka smoother on the device (mg_vanka_time_dev: events on the handle's stream) beside a
byte model and beside one Jacobi sweep (mg_time_op_dev_FP64, MG_K_SMOOTH) on the same operator in the same job.  3-D mixed
operator of tests/vanka_cases.py on m^3 cells (default 128).
    python profiles/vanka_measure.py [m] [out.json]"""
import ctypes as C
import json
import os
import sys
import time

import torch
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multigrid_jl_amd as mg   # noqa: E402
import vanka_cases as V         # noqa: E402

D = mg.device
REPS, WARM = 20, 3


def byte_model(A, n, bs):
    """Bytes one FULL_VANKA_RB iteration has to move, every operand from HBM once per use the caches cannot merge:
    every face row is read by the two cells that list it (value 8 B + column 4 B per entry, two row pointers per visit), a
    pressure row by one; the blocks once (4 B x bs^2 per cell); b once per row visit; x once per colour pass (the gathers of a
    pass re-read it from cache); the delta buffer written and read once; x read and written once per row visit in the apply."""
    cells = int(np.prod(n))
    nfaces = A.shape[0] - cells
    lens = np.diff(A.indptr)
    nnz_f, nnz_p = int(lens[:nfaces].sum()), int(lens[nfaces:].sum())
    visits = bs * cells
    rows = 12 * (2 * nnz_f + nnz_p) + 8 * visits
    blocks = 4 * bs * bs * cells
    vecs = 8 * visits + 8 * A.shape[0] * 2 ** len(n) + 16 * visits + 16 * visits
    return dict(rows=rows, blocks=blocks, vectors=vecs, total=rows + blocks + vecs)


def main():
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    n = [m, m, m]
    t0 = time.perf_counter()
    A = V.mixed_operator(n, True)
    blk = mg.setupVankaFacesPreconditioner(A, np.asarray(n), 0.6, True, mg.FULL_VANKA_RB)
    setup_s = time.perf_counter() - t0
    N = A.shape[0]
    lib = D.load_library()
    H = mg.vanka.vanka_handle(A, blk, np.asarray(n), True)
    h, info = H.h, H.info()
    b = torch.from_numpy(V.seeded(N, 1)).cuda()
    x = torch.zeros_like(b)
    torch.cuda.synchronize()
    ms = (C.c_double * REPS)()
    D._check(lib, lib.mg_vanka_time_dev(h, D._ptr(x), D._ptr(b), mg.FULL_VANKA_RB, WARM, REPS, ms), "mg_vanka_time_dev")
    ms = np.array(list(ms))
    H.close()
    model = byte_model(A, n, info[1])
    # one Jacobi sweep of the same operator: a two-level handle whose coarse level is a single unknown
    P = sp.csr_matrix((np.ones(1), (np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64))), shape=(N, 1))
    p = mg.getMGparam(np.float64, np.int64, 2, 1, 1, 1e-8, "Jac", 0.8, 1, 1, "V")
    p.As = [A, sp.csr_matrix((P.T @ A @ P))]
    p.Ps, p.Rs = [P], [sp.csr_matrix(P.T)]
    p.relaxPrecs = [0.8 / A.diagonal()]
    p.LU = spla.splu(sp.csc_matrix(p.As[1]))
    p.nrhs = 1
    dev = D.DeviceHierarchy(p)
    jac_ms, jac_bytes = dev.time_op(1, D.MG_K_SMOOTH, REPS)
    dev.close()
    rec = dict(n=n, rows=N, nnz=int(A.nnz), host_setup_s=setup_s, info=info, vanka_ms_median=float(np.median(ms)),
               vanka_ms_min=float(ms.min()), vanka_ms_max=float(ms.max()), model_bytes=model,
               model_GBps_at_median=model["total"] / (np.median(ms) * 1e-3) / 1e9, jacobi_ms=float(jac_ms), jacobi_bytes=float(jac_bytes),
               vanka_over_jacobi=float(np.median(ms) / jac_ms))
    print(json.dumps(rec), flush=True)
    if len(sys.argv) > 2:
        json.dump(rec, open(sys.argv[2], "w"), indent=1)


if __name__ == "__main__":
    main()
