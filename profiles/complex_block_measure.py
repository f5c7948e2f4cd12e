"""Blocks of right-hand sides on complex hierarchies against the single-vector entry points (the parent commit's only way to serve
k sources: k calls), on the problem of profiles/complex_single_measure.py: shifted Laplacian at 128^3 cells (k h = 0.25, damping
0.5, four levels, SPAI, V(2,1)), system operator with damping 0.05; CF64 and CF32 hierarchy.
    python profiles/complex_block_measure.py all [out.json]   for nrhs in 1, 2, 4, 8, 16: (a) ms per column of one block cycle
                                                              (mg_block_cycle_dev_CFP64) against nrhs calls of mg_cycle_dev_CFP64,
                                                              (b) ms per column of one block BiCGSTAB iteration against the single
                                                              driver's, (c) iterations to 1e-8 of both, (d) bytes the block work
                                                              set holds; one warm-up, then 5 repetitions, block and single
                                                              alternating inside every repetition
    python profiles/complex_block_measure.py trace            block cycles alone (CF64, every nrhs): the run to put under
                                                              rocprofv3 --kernel-trace --stats --output-format csv
    python profiles/complex_block_measure.py stats <kernel_stats.csv>   the SpMM kernel's instantiations: calls, total, average
CB_CELLS overrides the 128 (rehearsals), CB_NRHS the list of column counts."""
import csv
import json
import os
import re
import sys
import time

import torch
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multigrid_jl_amd as mg                    # noqa: E402
from complex_cases import complex_rhs, helmholtz  # noqa: E402

CELLS = int(os.environ.get("CB_CELLS", "128"))
NRHS = [int(t) for t in os.environ.get("CB_NRHS", "1,2,4,8,16").split(",")]
ITERS, REPS, WARM, CYCLES = 5, 5, 1, 10
TOL, MAXIT = 1e-8, 200
PRE, POST = 2, 1


def build(single):
    Ah, mesh = helmholtz(mg, [CELLS] * 3, 0.25, 0.5)
    p = mg.getMGparam(np.complex128, np.int64, 4, 8, ITERS, 0.0, "SPAI", 1.0, PRE, POST, "V", "NoMUMPS", 0.5, 0.0, singlePrecision=single)
    mg.MGsetup(Ah, mesh, p)
    return p


def work_set_bytes(p, k):
    """What cx_block_ensure and the block driver hold for k columns: four level blocks per level in the handle's precision, three
    ComplexF64 staging blocks, seven ComplexF64 Krylov blocks (the coarsest solve's work vectors are small and not counted)."""
    cb = np.dtype(p.VAL).itemsize
    n0 = p.As[0].shape[0]
    return sum(4 * A.shape[0] * k * cb for A in p.As) + (3 + 7) * n0 * k * 16


def sweep_model_bytes(p, k):
    """Byte model of one SMOOTH sweep of the fine level on k columns: the matrix stream once, x gathered, b read and x' written per
    column, d once per row."""
    cb = np.dtype(p.VAL).itemsize
    A = p.As[0]
    n = A.shape[0]
    return A.nnz * (cb + 4) + (n + 1) * 4 + n * cb + 3 * n * k * cb


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def measure(out_path):
    As, _ = helmholtz(mg, [CELLS] * 3, 0.25, 0.05)
    n = As.shape[0]
    out = dict(cells=CELLS, n=n, nrhs=NRHS, iters=ITERS, reps=REPS, cycles=CYCLES)
    for name, single in (("CF64", False), ("CF32", True)):
        p = build(single)
        dev = mg.device.DeviceHierarchy(p)
        dev.set_krylov_operator(As)
        rec = {}
        for k in NRHS:
            B = np.ascontiguousarray(np.stack([complex_rhs(n, 40 + j) for j in range(k)], axis=1))     # row-major [n][k]
            Bt = torch.from_numpy(B).cuda()
            Xt = torch.zeros_like(Bt)
            cols = [(torch.from_numpy(np.ascontiguousarray(B[:, j])).cuda(), torch.zeros(n, dtype=torch.complex128, device="cuda")) for j in range(k)]

            def block_cycles():
                for _ in range(CYCLES):
                    dev.block_cycle_dev(Bt, Xt, 1)

            def single_cycles():
                for _ in range(CYCLES):
                    for bt, xt in cols:
                        dev.cycle_dev(bt, xt, 1)

            def block_iters(tol=0.0, maxit=ITERS):
                Xt.zero_()
                return dev.block_bicgstab_dev_CFP64(Bt, Xt, tol, maxit)

            def single_iters(tol=0.0, maxit=ITERS):
                res = []
                for bt, xt in cols:
                    xt.zero_()
                    res.append(dev.bicgstab_dev(bt, xt, tol, maxit))
                return res

            t = dict(block_cycle=[], single_cycle=[], block_iter=[], single_iter=[])
            for rep in range(WARM + REPS):                       # block and single alternate inside every repetition
                a = timed(block_cycles)[0]
                b_ = timed(single_cycles)[0]
                c = timed(block_iters)[0]
                d = timed(single_iters)[0]
                if rep >= WARM:
                    t["block_cycle"].append(1e3 * a / (CYCLES * k))
                    t["single_cycle"].append(1e3 * b_ / (CYCLES * k))
                    t["block_iter"].append(1e3 * c / (ITERS * k))
                    t["single_iter"].append(1e3 * d / (ITERS * k))
            r = {w: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for w, v in t.items()}
            _, (flag, it, _rv) = timed(lambda: block_iters(TOL, MAXIT))
            X = Xt.cpu().numpy()
            r["block_to_tol"] = dict(count=it, flag=flag, worst_true_residual=float((np.linalg.norm(B - As @ X, axis=0) / np.linalg.norm(B, axis=0)).max()))
            _, runs = timed(lambda: single_iters(TOL, MAXIT))
            r["single_to_tol"] = dict(counts=[q[1] for q in runs], flags=[q[0] for q in runs])
            r["work_set_bytes"] = work_set_bytes(p, k)
            r["sweep_model_bytes_per_row_col"] = sweep_model_bytes(p, k) / (n * k)
            print(name, k, json.dumps(r), flush=True)
            rec[str(k)] = r
            del Bt, Xt, cols
            torch.cuda.empty_cache()
        out[name] = rec
        dev.close()
        mg.clear_(p)
    if out_path:
        json.dump(out, open(out_path, "w"), indent=1)


def trace():
    p = build(False)
    dev = mg.device.DeviceHierarchy(p)
    n = p.As[0].shape[0]
    for k in NRHS:
        Bt = torch.from_numpy(np.ascontiguousarray(np.stack([complex_rhs(n, 40 + j) for j in range(k)], axis=1))).cuda()
        Xt = torch.zeros_like(Bt)
        s, _ = timed(lambda: [dev.block_cycle_dev(Bt, Xt, 1) for _ in range(CYCLES)])
        print(f"nrhs {k}: {1e3 * s / CYCLES:.3f} ms per block cycle; fine SMOOTH model {sweep_model_bytes(p, k) / (n * k):.1f} B per row and column", flush=True)
    dev.close()


def stats(path):
    """Every cx_csr_stream_spmm instantiation of the trace.  One launch serves one nrhs; the trace runs CYCLES cycles per nrhs, so
    the per-nrhs split comes from the kernel trace itself (kernel_trace.csv), this table gives the totals."""
    for r in csv.DictReader(open(path)):
        name = r.get("Name") or r.get("KernelName") or ""
        if "cx_csr_stream_spmm" not in name and "cx_dscale_blk" not in name and "cx_dense_matblk" not in name:
            continue
        calls = int(r.get("Calls") or r.get("Count") or 0)
        total_ns = float(r.get("TotalDurationNs") or r.get("TotalNs") or r.get("Total") or 0.0)
        avg_ns = float(r.get("AverageNs") or r.get("Average") or 0.0)
        short = re.sub(r"mgk::|__attribute__\(\(ext_vector_type\(2\)\)\)", "", name)
        print(f"calls {calls:6d}  total {total_ns / 1e6:9.3f} ms  average {avg_ns / 1e3:8.1f} us  {short}")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    if mode == "stats":
        stats(sys.argv[2])
    elif mode == "trace":
        trace()
    else:
        measure(sys.argv[2] if len(sys.argv) > 2 else None)
