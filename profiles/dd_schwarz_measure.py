"""One sweep of the Schwarz preconditioner on the device (mg_dd_time_dev: events on the handle's stream) against what the
library offered before it: one mg_lu handle per sub-domain driven from the host with mg_lu_solve_dev_*, torch gathers for
residual and update.  3-D Poisson (complex: a damped Helmholtz shift of it) on 64 x 64 x 32 cells.
    python profiles/dd_schwarz_measure.py [all | batched | chipwide | batched_FP64 | ...] [out.json]
DD_NO_BASELINE=1 leaves the baseline out (kernel traces)."""
import ctypes as C
import json
import os
import sys
import time

import torch
import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multigrid_jl_amd as mg   # noqa: E402
import dd_cases                  # noqa: E402

D = mg.device
PJS = mg.ParallelJuliaSolver
REPS, WARM = 30, 5


def case(n, boxes, ov, cx):
    A, mesh, b = dd_cases.poisson(mg, n, seed=1)
    if cx:
        A = (A.astype(np.complex128) - (1.0 - 0.5j) * 0.25 * (A.diagonal().max() / 6) * sp.identity(A.shape[0])).tocsr()
        A.sort_indices()
        b = b + 1j * np.random.default_rng(9).standard_normal(A.shape[0])
    VAL = np.complex128 if cx else np.float64
    t0 = time.perf_counter()
    p = dd_cases.dd_param(mg, A, mesh, boxes, ov, VAL=VAL)
    setup_s = time.perf_counter() - t0
    return A, b, p, VAL, setup_s


def time_dd(A, b, p, VAL):
    lib = D.load_library()
    info = mg.DomainDecomposition.ddInfo(p, A)
    h = p._handle
    bd = torch.from_numpy(b).cuda()
    xd = torch.zeros_like(bd)
    torch.cuda.synchronize()
    ms = (C.c_double * REPS)()
    D._check(lib, lib.mg_dd_time_dev(h, D._ptr(bd), D._ptr(xd), A.shape[0], 0, WARM, REPS, ms), "mg_dd_time_dev")
    # the result of the first sweep, for the comparison with the baseline
    xd.zero_()
    torch.cuda.synchronize()
    mg.solveDDSerial(A, bd, xd, p, 1, 0)
    torch.cuda.synchronize()
    return np.array(list(ms)), info, xd.cpu().numpy()


def time_baseline(A, b, p, VAL):
    """What the parent commit offers: per sub-domain a torch gather of the residual, mg_lu_solve_dev on the sub-domain's own
    handle, a torch index_add; colours and order as the reference's loop."""
    lib = D.load_library()
    cx = VAL is np.complex128
    solve = lib.mg_lu_solve_dev_CFP64 if cx else lib.mg_lu_solve_dev_FP64
    subs = []
    for prec, g in zip(p.PrecParams, p.GlobalIndices):
        s = prec.Ainv
        if s._handle is None:
            PJS._upload_factors(s)
        I = g.astype(np.int64) - 1
        Ai = A[I].tocsr()
        rowid = torch.from_numpy(np.repeat(np.arange(len(I)), np.diff(Ai.indptr))).cuda()
        cols = torch.from_numpy(Ai.indices.astype(np.int64)).cuda()
        vals = torch.from_numpy(Ai.data).cuda()
        It = torch.from_numpy(I).cuda()
        subs.append((mg.cellColor(prec.i), s._handle, It, (rowid, cols, vals), torch.zeros(len(I), dtype=vals.dtype, device="cuda"), len(I)))
    order = [k for c in range(1, 9) for k in range(len(subs)) if subs[k][0] == c]
    bd = torch.from_numpy(b).cuda()
    xd = torch.zeros_like(bd)

    def sweep():
        for k in order:
            _, h, It, rows, t, n_i = subs[k]
            rowid, cols, vals = rows
            r = bd[It]
            prod = vals * xd[cols]
            if cx:
                torch.view_as_real(r).index_add_(0, rowid, torch.view_as_real(prod), alpha=-1.0)
            else:
                r.index_add_(0, rowid, prod, alpha=-1.0)
            torch.cuda.current_stream().synchronize()           # the applier runs on a stream of its own
            D._check(lib, solve(h, D._ptr(r), D._ptr(t), n_i, 1, 0), "mg_lu_solve_dev")   # returns after its stream drained
            xd[It] += t

    sweep()
    torch.cuda.synchronize()
    x1 = xd.cpu().numpy().copy()
    for _ in range(2):
        sweep()
    ms = []
    for _ in range(10):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sweep()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    for prec in p.PrecParams:
        prec.Ainv.close()
    return np.array(ms), x1


def main():
    only = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] != "all" else None
    out = {}
    shapes = {"batched": ([64, 64, 32], [8, 8, 4], [1, 1, 1]), "chipwide": ([64, 64, 32], [4, 4, 2], [2, 2, 2])}
    for name, (n, boxes, ov) in shapes.items():
        for cx in (False, True):
            key = f"{name}_{'CFP64' if cx else 'FP64'}"
            if only and only != key and only != name:
                continue
            A, b, p, VAL, setup_s = case(n, boxes, ov, cx)
            ms, info, x_dd = time_dd(A, b, p, VAL)
            rec = dict(n=n, boxes=boxes, overlap=ov, rows=int(A.shape[0]), max_sub_rows=int(max(len(g) for g in p.GlobalIndices)),
                       host_setup_s=setup_s, info=info, dd_ms_median=float(np.median(ms)), dd_ms_min=float(ms.min()), dd_ms_max=float(ms.max()))
            print(key, "dd only", json.dumps(rec), flush=True)
            if not os.environ.get("DD_NO_BASELINE"):
                bms, x_b = time_baseline(A, b, p, VAL)
                rec.update(base_ms_median=float(np.median(bms)), base_ms_min=float(bms.min()), base_ms_max=float(bms.max()),
                           rel_diff_first_sweep=float(np.abs(x_dd - x_b).max() / np.abs(x_b).max()))
                rec["ratio_base_over_dd"] = rec["base_ms_median"] / rec["dd_ms_median"]
            print(key, json.dumps(rec), flush=True)
            out[key] = rec
            p.close()
            if len(sys.argv) > 2:
                json.dump(out, open(sys.argv[2], "w"), indent=1)


if __name__ == "__main__":
    main()
