"""The ComplexF32 hierarchy inside the ComplexF64 Krylov drivers against the ComplexF64 hierarchy (this tree's library and,
when CS_PARENT_LIB names the parent commit's libmgvcycle.so, that one too), on the problem of profiles/complex_krylov_measure.py:
shifted Laplacian at 128^3 cells (k h = 0.25, damping 0.5, four levels, SPAI, V(2,1)), system operator with damping 0.05.
    python profiles/complex_single_measure.py all [out.json]     (a) ms per BiCGSTAB iteration and per FGMRES(10) inner step,
                                                                 (b) ms per cycle alone, (c) iterations to 1e-8, (d) HBM held by
                                                                 each hierarchy; one warm-up, then 5 repetitions, the hierarchies
                                                                 alternating inside every repetition
    python profiles/complex_single_measure.py trace              cycles alone, both precisions: the run to put under
                                                                 rocprofv3 --kernel-trace --stats
    python profiles/complex_single_measure.py stats <kernel_stats.csv>   (e) the stream kernel's instantiations, time and model bytes
CS_CELLS overrides the 128 (rehearsals)."""
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

CELLS = int(os.environ.get("CS_CELLS", "128"))
ITERS, INNER, REPS, WARM, CYCLES = 10, 10, 5, 1, 20
TOL, MAXIT = 1e-8, 200
PRE, POST = 2, 1


def build(single):
    Ah, mesh = helmholtz(mg, [CELLS] * 3, 0.25, 0.5)
    p = mg.getMGparam(np.complex128, np.int64, 4, 8, ITERS, 0.0, "SPAI", 1.0, PRE, POST, "V", "NoMUMPS", 0.5, 0.0, singlePrecision=single)
    mg.MGsetup(Ah, mesh, p)
    return p


def hierarchy_bytes(p):
    """HBM held by the uploaded hierarchy, from the array sizes: values + column indices + row pointers + row blocks of every
    operator, relaxPrecs, the four level vectors (b, r, x, x'); the coarsest solve (double in both) is not counted."""
    cb = np.dtype(p.VAL).itemsize
    rb = cb // 2
    total = 0
    for l, A in enumerate(p.As):
        n = A.shape[0]
        total += A.nnz * (cb + 4) + (n + 1) * 4 + 4 * n * cb
        if l < len(p.Ps):
            total += n * cb
            for T in (p.Ps[l], p.Rs[l]):
                total += T.nnz * (rb + 4) + (T.shape[0] + 1) * 4
    return total


def cycle_model_bytes(p):
    """Bytes one V(PRE, POST) cycle moves through the stream kernel, by (mode, operator): values + indices of the operator, the
    gathered vector once, the row operands and the result (the byte model of DESIGN.md)."""
    cb = np.dtype(p.VAL).itemsize
    rb = cb // 2
    out = {"SMOOTH A": 0, "RESID A": 0, "AXPBY R": 0, "AXPBY P": 0}
    for l in range(len(p.Ps)):
        A, P, R = p.As[l], p.Ps[l], p.Rs[l]
        n, nc = A.shape[0], P.shape[1]
        mat = A.nnz * (cb + 4)
        out["SMOOTH A"] += (PRE - 1 + POST) * (mat + 4 * n * cb)         # x gathered, b, d read, x' written (the first pre-sweep is x = d.*b)
        out["RESID A"] += mat + 3 * n * cb
        out["AXPBY R"] += R.nnz * (rb + 4) + n * cb + nc * cb
        out["AXPBY P"] += P.nnz * (rb + 4) + nc * cb + 2 * n * cb
    return out


def run(dev, method, bt, xt, tol, maxit):
    xt.zero_()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if method == "bicgstab":
        flag, it, _ = dev.bicgstab_dev(bt, xt, tol, maxit)
    else:
        flag, it, _ = dev.fgmres_dev(bt, xt, INNER, tol, maxit)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, it, flag


def cycles(dev, bt, xt, count=CYCLES):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(count):
        dev.cycle_dev(bt, xt, 1)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / count


def load_other(path):
    """Another build of the library (the parent commit's): the symbols it has, with this tree's signatures."""
    import ctypes
    lib = ctypes.CDLL(path)
    for name, (res, args) in mg.device.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def hierarchies(with_parent):
    """name -> (param, device hierarchy); 'parent CF64' runs the library CS_PARENT_LIB names on the same ComplexF64 param."""
    t0 = time.perf_counter()
    p64, p32 = build(False), build(True)
    setup_s = time.perf_counter() - t0
    As, _ = helmholtz(mg, [CELLS] * 3, 0.25, 0.05)
    devs = {}
    parent = os.environ.get("CS_PARENT_LIB") if with_parent else None
    if parent:
        mine = mg.device.load_library()
        mg.device._lib = load_other(parent)                      # (a second copy of the library, bound to this one hierarchy)
        try:
            devs["parent CF64"] = (p64, mg.device.DeviceHierarchy(p64))
        finally:
            mg.device._lib = mine
    devs["CF64"] = (p64, mg.device.DeviceHierarchy(p64))
    devs["CF32"] = (p32, mg.device.DeviceHierarchy(p32))
    for _, d in devs.values():
        d.set_krylov_operator(As)
    return devs, As, setup_s


def measure(out_path):
    devs, As, setup_s = hierarchies(True)
    n = As.shape[0]
    b = complex_rhs(n, 21)
    bt = torch.from_numpy(b).cuda()
    xt = torch.zeros(n, dtype=torch.complex128, device="cuda")
    out = dict(cells=CELLS, n=n, setup_s=setup_s, iters=ITERS, inner=INNER, reps=REPS,
               hbm_bytes={k: hierarchy_bytes(p) for k, (p, _) in devs.items()})
    times = {k: dict(bicgstab=[], fgmres=[], cycle=[]) for k in devs}
    for rep in range(WARM + REPS):                               # the hierarchies alternate inside every repetition
        for k, (_, d) in devs.items():
            s, it, _ = run(d, "bicgstab", bt, xt, 0.0, ITERS)
            sg, itg, _ = run(d, "fgmres", bt, xt, 0.0, 1)
            sc = cycles(d, bt, xt)
            if rep >= WARM:
                times[k]["bicgstab"].append(1e3 * s / it)
                times[k]["fgmres"].append(1e3 * sg / itg)
                times[k]["cycle"].append(1e3 * sc)
    for k, (_, d) in devs.items():
        rec = {}
        for what, v in times[k].items():
            rec[what] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
        for method in ("bicgstab", "fgmres"):                    # (c) iterations to 1e-8
            _, it, flag = run(d, method, bt, xt, TOL, MAXIT)
            x = xt.cpu().numpy()
            rec[f"{method}_to_tol"] = dict(count=it, flag=flag, true_residual=float(np.linalg.norm(b - As @ x) / np.linalg.norm(b)))
        print(k, json.dumps(rec), flush=True)
        out[k] = rec
    if out_path:
        json.dump(out, open(out_path, "w"), indent=1)
    for _, d in devs.values():
        d.close()


def trace():
    devs, As, _ = hierarchies(False)
    n = As.shape[0]
    bt = torch.from_numpy(complex_rhs(n, 21)).cuda()
    xt = torch.zeros(n, dtype=torch.complex128, device="cuda")
    for k, (p, d) in devs.items():
        print(k, f"{1e3 * cycles(d, bt, xt):.3f} ms per cycle;", "model bytes per cycle:", json.dumps(cycle_model_bytes(p)), flush=True)
        d.close()


def stats(path):
    """Every cx_csr_stream_spmv instantiation of the trace: calls, total and average time.  The cycles of `trace` are the only
    callers, CYCLES + 0 per precision, so total time / CYCLES is the kernel's time per cycle to set against cycle_model_bytes."""
    rows = list(csv.DictReader(open(path)))
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        if "cx_csr_stream_spmv" not in name and "cx_narrow" not in name and "cx_widen" not in name and "cx_dscale" not in name:
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
