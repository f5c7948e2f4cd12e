"""ComplexF64 BiCGSTAB and FGMRES(10) on the device (mg_bicgstab_dev_CFP64 / mg_fgmres_dev_CFP64) against the only route the
library offered before them: the same algorithms driven from the host - numpy vectors, scipy's product with the system operator -
with getMultigridPreconditioner(param, b) as M (every application sends a complex vector over PCIe and back).
Shifted-Laplacian hierarchy at 128^3 cells (k h = 0.25, damping 0.5, four levels, SPAI, V(2,1)), system operator with damping 0.05.
    python profiles/complex_krylov_measure.py [all | device] [out.json]      time per iteration, median of alternating repetitions
    python profiles/complex_krylov_measure.py stats <kernel_stats.csv>         each pass's time and bytes-per-element model from a
                                                                               rocprofv3 --kernel-trace --stats run of `device`
CK_CELLS overrides the 128 (rehearsals)."""
import csv
import json
import os
import sys
import time

import torch
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multigrid_jl_amd as mg                    # noqa: E402
import complex_krylov_oracle as ck               # noqa: E402  (the host-driven algorithms: numpy restatements of bicgstb / fgmres)
from complex_cases import complex_rhs, helmholtz  # noqa: E402

CELLS = int(os.environ.get("CK_CELLS", "128"))
ITERS, INNER, REPS, WARM = 10, 10, 5, 1
# bytes per complex element of each pass (csrc/mg_cxvec.hpp), by the name of its Op in the kernel's symbol
MODEL = {"OpCDots": 32, "OpCScale": 32, "OpCBicgP": 64, "OpCBicgS": 48, "OpCBicgTS": 32, "OpCBicgXR": 128, "OpCMgsStep": 64,
         "OpCGsUpdate": None}   # gs_update: 16 (m + 2), m varies by launch


def setup():
    t0 = time.perf_counter()
    Ah, mesh = helmholtz(mg, [CELLS] * 3, 0.25, 0.5)
    p = mg.getMGparam(np.complex128, np.int64, 4, 8, ITERS, 0.0, "SPAI", 1.0, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(Ah, mesh, p)
    As, _ = helmholtz(mg, [CELLS] * 3, 0.25, 0.05)
    b = complex_rhs(Ah.shape[0], 21)
    dev = mg.to_device(p)
    dev.set_krylov_operator(As)
    return p, dev, As, b, time.perf_counter() - t0


def device_run(dev, method, bt, xt):
    """tol = 0: exactly ITERS iterations / one restart cycle of INNER steps.  Returns (seconds, iterations)."""
    xt.zero_()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if method == "bicgstab":
        flag, it, _ = dev.bicgstab_dev(bt, xt, 0.0, ITERS)
    else:
        flag, it, _ = dev.fgmres_dev(bt, xt, INNER, 0.0, 1)
    torch.cuda.synchronize()                                   # (the drivers return with their stream drained)
    return time.perf_counter() - t0, it


def host_run(p, As, method, b):
    MMG = mg.getMultigridPreconditioner(p, b)
    M = lambda v: MMG(np.ascontiguousarray(v)).copy()          # the closure returns its own buffer
    Afun = lambda v: As @ v
    t0 = time.perf_counter()
    if method == "bicgstab":
        _, flag, it, _ = ck.bicgstb(Afun, b, 0.0, ITERS, M)
    else:
        _, flag, it, _ = ck.fgmres(Afun, b, INNER, 0.0, 1, M)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, it


def measure(only_device, out_path):
    p, dev, As, b, setup_s = setup()
    n = b.shape[0]
    bt = torch.from_numpy(b).cuda()
    xt = torch.zeros(n, dtype=torch.complex128, device="cuda")
    out = dict(cells=CELLS, n=n, levels=len(p.As), setup_s=setup_s, iters=ITERS, inner=INNER, reps=REPS)
    for method in ("bicgstab", "fgmres"):
        dms, hms = [], []
        for rep in range(WARM + REPS):                          # alternating: device, host, device, host ...
            s, it = device_run(dev, method, bt, xt)
            if rep >= WARM:
                dms.append(1e3 * s / it)
            if not only_device:
                s, ith = host_run(p, As, method, b)
                assert ith == it
                if rep >= WARM:
                    hms.append(1e3 * s / ith)
        rec = dict(iterations=it, device_ms_per_iter=float(np.median(dms)), device_min=float(min(dms)), device_max=float(max(dms)))
        if hms:
            rec.update(host_ms_per_iter=float(np.median(hms)), host_min=float(min(hms)), host_max=float(max(hms)))
            rec["host_over_device"] = rec["host_ms_per_iter"] / rec["device_ms_per_iter"]
        print(method, json.dumps(rec), flush=True)
        out[method] = rec
    if out_path:
        json.dump(out, open(out_path, "w"), indent=1)
    mg.clear_(p)


def stats(path):
    n = (CELLS + 1) ** 3
    rows = list(csv.DictReader(open(path)))
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        for op, bpe in MODEL.items():
            if op in name:
                avg_ns = float(r.get("AverageNs") or r.get("Average") or 0.0)
                calls = r.get("Calls") or r.get("Count")
                rate = f"{bpe * n / avg_ns:.0f} GB/s of {bpe} B/element" if bpe and avg_ns else "bytes vary by launch"
                print(f"{op:12s} calls {calls:>5s}  average {avg_ns / 1e3:8.1f} us  {rate}")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    if mode == "stats":
        stats(sys.argv[2])
    else:
        measure(mode == "device", sys.argv[2] if len(sys.argv) > 2 else None)
