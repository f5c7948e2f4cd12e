"""ComplexF64 Jac-GMRES smoothing and the K-cycle on the device, on the problem of profiles/complex_krylov_measure.py: shifted
Laplacian at 128^3 cells (k h = 0.25, damping 0.5, four levels, omega 0.8), system operator with damping 0.05.
    python profiles/complex_kcycle_measure.py all [out.json]        ms per cycle of V(2,1) / W(2,1) Jac, V(2,1) Jac-GMRES, K(2,1) Jac
                                                                    and K(2,1) Jac-GMRES (one warm-up, then 5 rounds; the schedules
                                                                    alternate inside every round), then BiCGSTAB and FGMRES(10) to
                                                                    1e-8 with each hierarchy as preconditioner: count, flag, seconds
    python profiles/complex_kcycle_measure.py regress OTHER_ROOT [out.json]
                                                                    no regression of what exists: the V(2,1) Jac cycle and the 4-column
                                                                    block cycle of THIS tree against another built tree (the parent
                                                                    commit), one child process each, rounds alternating between them
    python profiles/complex_kcycle_measure.py trace                 V(2,1) Jac and V(2,1) Jac-GMRES cycles alone: the run to put under
                                                                    rocprofv3 --kernel-trace --stats --output-format csv
    python profiles/complex_kcycle_measure.py stats <kernel_stats.csv>   the stream kernel's instantiations: calls, total, average
Times are wall-clock around CYCLES cycles between device synchronisations (a Jac-GMRES / K cycle synchronises the host itself, so
its host time is part of what it costs).  CK_CELLS overrides the 128 (rehearsals)."""
import csv
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "child" else HERE
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CELLS = int(os.environ.get("CK_CELLS", "128"))
REPS, WARM, CYCLES = 5, 1, 10
TOL, MAXIT = 1e-8, 200
SCHEDULES = [("Jac", "V"), ("Jac", "W"), ("Jac-GMRES", "V"), ("Jac", "K"), ("Jac-GMRES", "K")]


def build(mg, relax, cyc):
    from complex_cases import helmholtz
    Ah, mesh = helmholtz(mg, [CELLS] * 3, 0.25, 0.5)
    p = mg.getMGparam(np.complex128, np.int64, 4, 8, MAXIT, TOL, relax, 0.8, 2, 1, cyc, "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(Ah, mesh, p)
    return p


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def stat(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def measure(out_path):
    import torch
    import multigrid_jl_amd as mg
    from complex_cases import complex_rhs, helmholtz
    As, _ = helmholtz(mg, [CELLS] * 3, 0.25, 0.05)
    n = As.shape[0]
    b = complex_rhs(n, 21)
    bt = torch.from_numpy(b).cuda()
    xt = torch.zeros(n, dtype=torch.complex128, device="cuda")
    devs = {}
    for s in SCHEDULES:
        p = build(mg, *s)
        devs[s] = (p, mg.device.DeviceHierarchy(p))
        devs[s][1].set_krylov_operator(As)
    t = {s: [] for s in SCHEDULES}
    for rep in range(WARM + REPS):                               # the schedules alternate inside every round
        for s in SCHEDULES:
            dev = devs[s][1]
            sec = timed(torch, lambda: [dev.cycle_dev(bt, xt, 1) for _ in range(CYCLES)])[0]
            if rep >= WARM:
                t[s].append(1e3 * sec / CYCLES)
    out = dict(cells=CELLS, n=n, cycles=CYCLES, reps=REPS, cycle_ms={}, krylov={})
    for s in SCHEDULES:
        out["cycle_ms"]["%s %s(2,1)" % s] = stat(t[s])
        print("cycle", s, json.dumps(stat(t[s])), flush=True)
    for s in SCHEDULES:
        dev = devs[s][1]
        rec = {}
        for name, run in (("bicgstab", lambda x: dev.bicgstab_dev(bt, x, TOL, MAXIT)), ("fgmres10", lambda x: dev.fgmres_dev(bt, x, 10, TOL, MAXIT))):
            runs = []
            for rep in range(WARM + 3):
                xt.zero_()
                sec, (flag, it, rv) = timed(torch, lambda: run(xt))
                if rep >= WARM:
                    runs.append(sec)
            x = xt.cpu().numpy()
            rec[name] = dict(flag=flag, count=it, seconds=stat(runs), true_residual=float(np.linalg.norm(b - As @ x) / np.linalg.norm(b)))
        out["krylov"]["%s %s(2,1)" % s] = rec
        print("krylov", s, json.dumps(rec), flush=True)
    for p, dev in devs.values():
        dev.close()
    if out_path:
        json.dump(out, open(out_path, "w"), indent=1)


def child():
    """One tree's V(2,1) Jac hierarchy; a line on stdin names what to time ("cycle" / "block"), the answer is ms per cycle."""
    import torch
    import multigrid_jl_amd as mg
    from complex_cases import complex_rhs
    p = build(mg, "Jac", "V")
    dev = mg.device.DeviceHierarchy(p)
    n = p.As[0].shape[0]
    bt = torch.from_numpy(complex_rhs(n, 21)).cuda()
    xt = torch.zeros_like(bt)
    Bt = torch.from_numpy(np.ascontiguousarray(np.stack([complex_rhs(n, 40 + j) for j in range(4)], axis=1))).cuda()
    Xt = torch.zeros_like(Bt)
    print("ready", flush=True)
    for line in sys.stdin:
        what = line.strip()
        if what == "cycle":
            sec = timed(torch, lambda: [dev.cycle_dev(bt, xt, 1) for _ in range(CYCLES)])[0]
        elif what == "block":
            sec = timed(torch, lambda: [dev.block_cycle_dev(Bt, Xt, 1) for _ in range(CYCLES)])[0]
        else:
            break
        print(1e3 * sec / CYCLES, flush=True)
    dev.close()


def regress(other, out_path):
    kids = {name: subprocess.Popen([sys.executable, os.path.abspath(__file__), "child", root], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                   text=True, bufsize=1) for name, root in (("this", HERE), ("other", other))}
    for k in kids.values():
        assert k.stdout.readline().strip() == "ready"
    t = {(name, what): [] for name in kids for what in ("cycle", "block")}
    for rep in range(WARM + 2 * REPS):                           # rounds alternate between the two trees
        for what in ("cycle", "block"):
            for name, k in kids.items():
                k.stdin.write(what + "\n")
                ms = float(k.stdout.readline())
                if rep >= WARM:
                    t[(name, what)].append(ms)
    for k in kids.values():
        k.stdin.write("quit\n")
        k.wait(timeout=60)
    out = {"%s %s" % key: stat(v) for key, v in t.items()}
    for key, v in out.items():
        print(key, json.dumps(v), flush=True)
    if out_path:
        json.dump(out, open(out_path, "w"), indent=1)


def trace():
    import torch
    import multigrid_jl_amd as mg
    from complex_cases import complex_rhs
    for s in (("Jac", "V"), ("Jac-GMRES", "V")):
        p = build(mg, *s)
        dev = mg.device.DeviceHierarchy(p)
        n = p.As[0].shape[0]
        bt = torch.from_numpy(complex_rhs(n, 21)).cuda()
        xt = torch.zeros_like(bt)
        sec = timed(torch, lambda: [dev.cycle_dev(bt, xt, 1) for _ in range(CYCLES)])[0]
        print("%s %s(2,1): %.3f ms per cycle" % (s + (1e3 * sec / CYCLES,)), flush=True)
        dev.close()


def stats(path):
    """Every cx_csr_stream_spmv instantiation of the trace (template argument 1: 0 AXPBY, 1 RESID, 2 SMOOTH, 3 GRAM)."""
    for r in csv.DictReader(open(path)):
        name = r.get("Name") or r.get("KernelName") or ""
        if "cx_csr_stream_spmv" not in name and "krv_final" not in name and "cxv_pass" not in name:
            continue
        calls = int(r.get("Calls") or r.get("Count") or 0)
        total_ns = float(r.get("TotalDurationNs") or r.get("TotalNs") or r.get("Total") or 0.0)
        avg_ns = float(r.get("AverageNs") or r.get("Average") or 0.0)
        short = re.sub(r"mgk::|__attribute__\(\(ext_vector_type\(2\)\)\)", "", name)
        print(f"calls {calls:6d}  total {total_ns / 1e6:9.3f} ms  average {avg_ns / 1e3:8.1f} us  {short}")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    if mode == "child":
        child()
    elif mode == "regress":
        regress(os.path.abspath(sys.argv[2]), sys.argv[3] if len(sys.argv) > 3 else None)
    elif mode == "stats":
        stats(sys.argv[2])
    elif mode == "trace":
        trace()
    else:
        measure(sys.argv[2] if len(sys.argv) > 2 else None)
