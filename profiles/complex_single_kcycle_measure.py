"""Jac-GMRES smoothing and the K-cycle on a ComplexF32 hierarchy (``singleKcycle=True``) against the same schedules on the ComplexF64
hierarchy, on the problem of profiles/complex_kcycle_measure.py: shifted Laplacian at 128^3 cells (k h = 0.25, damping 0.5, four levels,
omega 0.8), system operator with damping 0.05.  The numbers of profiles/complex_single_kcycle.md.
    python profiles/complex_single_kcycle_measure.py all [out.json]     HBM held by each hierarchy; ms per cycle of V(2,1) Jac,
                                                                        V(2,1) Jac-GMRES, K(2,1) Jac and K(2,1) Jac-GMRES on both (one
                                                                        warm-up, then 5 rounds; precisions and schedules alternate
                                                                        inside every round); BiCGSTAB and FGMRES(10) to 1e-8 with each
                                                                        as preconditioner: count, flag, seconds, seconds per step
    python profiles/complex_single_kcycle_measure.py regress OTHER_ROOT [out.json]
                                                                        the paths the change leaves alone, THIS tree against another
                                                                        built tree (the parent commit), one child process each, rounds
                                                                        alternating: ComplexF64 V(2,1) Jac and K(2,1) Jac-GMRES cycles,
                                                                        the ComplexF32 V(2,1) Jac cycle, the 4-column block cycle -
                                                                        ms per cycle and a digest of the result's bytes
    python profiles/complex_single_kcycle_measure.py trace              V(2,1) Jac-GMRES cycles in both precisions and V(2,1) Jac in
                                                                        single: the run to put under rocprofv3 --kernel-trace
                                                                        --output-format csv
    python profiles/complex_single_kcycle_measure.py stats <kernel_trace.csv>
                                                                        the fine-level launches (the largest grid of each kernel) of
                                                                        the stream kernel's GRAM / SMOOTH / RESID instantiations and of
                                                                        the relaxation's passes: calls, median, min - max in us
One hierarchy is set up per precision; the schedules are switched on the resident hierarchy (sync_schedule: Jac and Jac-GMRES share
relaxPrecs).  Times are wall-clock around CYCLES cycles between device synchronisations (a Jac-GMRES / K cycle synchronises the host
itself, so its host time is part of what it costs).  CK_CELLS overrides the 128 (rehearsals)."""
import csv
import hashlib
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
SCHEDULES = [("Jac", "V"), ("Jac-GMRES", "V"), ("Jac", "K"), ("Jac-GMRES", "K")]


def build(mg, single, relax="Jac", cyc="V", flag=True):
    from complex_cases import helmholtz
    Ah, mesh = helmholtz(mg, [CELLS] * 3, 0.25, 0.5)
    kw = dict(singlePrecision=True, singleKcycle=True) if single and flag else dict(singlePrecision=True) if single else {}
    p = mg.getMGparam(np.complex128, np.int64, 4, 8, MAXIT, TOL, relax, 0.8, 2, 1, cyc, "NoMUMPS", 0.5, 0.0, **kw)
    mg.MGsetup(Ah, mesh, p)
    return p


def switch(p, dev, relax, cyc):
    p.relaxType, p.cycleType = relax, cyc
    dev.sync_schedule(p)


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
    torch.cuda.init()
    As, _ = helmholtz(mg, [CELLS] * 3, 0.25, 0.05)
    n = As.shape[0]
    b = complex_rhs(n, 21)
    bt = torch.from_numpy(b).cuda()
    xt = torch.zeros(n, dtype=torch.complex128, device="cuda")
    out = dict(cells=CELLS, n=n, nnz=int(As.nnz), cycles=CYCLES, reps=REPS, hbm_mib={}, cycle_ms={}, krylov={})
    devs = {}
    for prec in ("CF64", "CF32"):
        p = build(mg, prec == "CF32")
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        dev = mg.device.DeviceHierarchy(p)
        out["hbm_mib"][prec + " V(2,1) Jac"] = (free0 - torch.cuda.mem_get_info()[0]) / 2 ** 20
        switch(p, dev, "Jac-GMRES", "K")
        out["hbm_mib"][prec + " K(2,1) Jac-GMRES"] = (free0 - torch.cuda.mem_get_info()[0]) / 2 ** 20
        free1 = torch.cuda.mem_get_info()[0]
        dev.set_krylov_operator(As)
        out["hbm_mib"][prec + " Krylov operator and vectors"] = (free1 - torch.cuda.mem_get_info()[0]) / 2 ** 20
        devs[prec] = (p, dev)
    print("hbm", json.dumps(out["hbm_mib"]), flush=True)
    keys = [(prec, s) for s in SCHEDULES for prec in ("CF64", "CF32")]
    t = {k: [] for k in keys}
    for rep in range(WARM + REPS):                               # precisions and schedules alternate inside every round
        for prec, s in keys:
            p, dev = devs[prec]
            switch(p, dev, *s)
            dev.cycle_dev(bt, xt, 1)                             # (the first cycle behind a schedule change is not timed)
            sec = timed(torch, lambda: [dev.cycle_dev(bt, xt, 1) for _ in range(CYCLES)])[0]
            if rep >= WARM:
                t[(prec, s)].append(1e3 * sec / CYCLES)
    for prec, s in keys:
        name = "%s %s %s(2,1)" % ((prec,) + s)
        out["cycle_ms"][name] = stat(t[(prec, s)])
        print("cycle", name, json.dumps(out["cycle_ms"][name]), flush=True)
    for prec, s in keys:
        p, dev = devs[prec]
        switch(p, dev, *s)
        rec = {}
        for name, run in (("bicgstab", lambda x: dev.bicgstab_dev(bt, x, TOL, MAXIT)), ("fgmres10", lambda x: dev.fgmres_dev(bt, x, 10, TOL, MAXIT))):
            runs = []
            for rep in range(WARM + 3):
                xt.zero_()
                sec, (flag, it, rv) = timed(torch, lambda: run(xt))
                if rep >= WARM:
                    runs.append(sec)
            x = xt.cpu().numpy()
            rec[name] = dict(flag=flag, count=it, seconds=stat(runs), ms_per_step=1e3 * float(np.median(runs)) / max(it, 1),
                             true_residual=float(np.linalg.norm(b - As @ x) / np.linalg.norm(b)))
        name = "%s %s %s(2,1)" % ((prec,) + s)
        out["krylov"][name] = rec
        print("krylov", name, json.dumps(rec), flush=True)
    for p, dev in devs.values():
        dev.close()
    if out_path:
        json.dump(out, open(out_path, "w"), indent=1)


def child():
    """One tree's hierarchies; a line on stdin names what to time, the answer is ms per cycle and a digest of the result."""
    import torch
    import multigrid_jl_amd as mg
    from complex_cases import complex_rhs
    pd, ps = build(mg, False), build(mg, True, flag=False)
    dd, ds = mg.device.DeviceHierarchy(pd), mg.device.DeviceHierarchy(ps)
    n = pd.As[0].shape[0]
    bt = torch.from_numpy(complex_rhs(n, 21)).cuda()
    xt = torch.zeros_like(bt)
    Bt = torch.from_numpy(np.ascontiguousarray(np.stack([complex_rhs(n, 40 + j) for j in range(4)], axis=1))).cuda()
    Xt = torch.zeros_like(Bt)
    digest = lambda a: hashlib.sha1(a.cpu().numpy().tobytes()).hexdigest()[:16]
    print("ready", flush=True)
    for line in sys.stdin:
        what = line.strip()
        if what in ("cf64_v_jac", "cf64_k_jacgmres"):
            switch(pd, dd, *(("Jac", "V") if what == "cf64_v_jac" else ("Jac-GMRES", "K")))
            dd.cycle_dev(bt, xt, 1)
            sec = timed(torch, lambda: [dd.cycle_dev(bt, xt, 1) for _ in range(CYCLES)])[0]
            res = xt
        elif what == "cf32_v_jac":
            sec = timed(torch, lambda: [ds.cycle_dev(bt, xt, 1) for _ in range(CYCLES)])[0]
            res = xt
        elif what == "cf64_block4":
            switch(pd, dd, "Jac", "V")
            dd.block_cycle_dev(Bt, Xt, 1)
            sec = timed(torch, lambda: [dd.block_cycle_dev(Bt, Xt, 1) for _ in range(CYCLES)])[0]
            res = Xt
        else:
            break
        print(1e3 * sec / CYCLES, digest(res), flush=True)
    dd.close()
    ds.close()


WHATS = ("cf64_v_jac", "cf64_k_jacgmres", "cf32_v_jac", "cf64_block4")


def regress(other, out_path):
    kids = {name: subprocess.Popen([sys.executable, os.path.abspath(__file__), "child", root], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                   text=True, bufsize=1) for name, root in (("this", HERE), ("other", other))}
    for k in kids.values():
        assert k.stdout.readline().strip() == "ready"
    t = {(name, what): [] for name in kids for what in WHATS}
    bits = {}
    for rep in range(WARM + REPS):                               # rounds alternate between the two trees
        for what in WHATS:
            for name, k in kids.items():
                k.stdin.write(what + "\n")
                ms, dig = k.stdout.readline().split()
                bits.setdefault(what, {}).setdefault(name, set()).add(dig)
                if rep >= WARM:
                    t[(name, what)].append(float(ms))
    for k in kids.values():
        k.stdin.write("quit\n")
        k.wait(timeout=120)
    out = {"%s %s" % key: stat(v) for key, v in t.items()}
    for what in WHATS:
        same = bits[what]["this"] == bits[what]["other"] and len(bits[what]["this"]) == 1
        out["same bits " + what] = bool(same)
    for key, v in out.items():
        print(key, json.dumps(v), flush=True)
    if out_path:
        json.dump(out, open(out_path, "w"), indent=1)


def trace():
    import torch
    import multigrid_jl_amd as mg
    from complex_cases import complex_rhs
    for single in (False, True):
        p = build(mg, single)
        dev = mg.device.DeviceHierarchy(p)
        n = p.As[0].shape[0]
        bt = torch.from_numpy(complex_rhs(n, 21)).cuda()
        xt = torch.zeros_like(bt)
        for s in (("Jac-GMRES", "V"), ("Jac", "V")):
            switch(p, dev, *s)
            sec = timed(torch, lambda: [dev.cycle_dev(bt, xt, 1) for _ in range(CYCLES)])[0]
            print("%s %s %s(2,1): %.3f ms per cycle" % (("CF32" if single else "CF64",) + s + (1e3 * sec / CYCLES,)), flush=True)
        dev.close()


def stats(path):
    """Per kernel of the relaxation: the launches on the largest grid (the fine level) - calls, median, min - max.  Template argument 1
    of cx_csr_stream_spmv: 0 AXPBY, 1 RESID, 2 SMOOTH, 3 GRAM; the last argument is the pair type (double2 / float2)."""
    groups = {}
    for r in csv.DictReader(open(path)):
        name = r.get("Kernel_Name") or r.get("Name") or ""
        if not re.search(r"cx_csr_stream_spmv|cx_dscale_sumsq|cxv_pass|krv_final", name):
            continue
        grid = int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)
        dur = (float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e3
        groups.setdefault(name, {}).setdefault(grid, []).append(dur)
    for name in sorted(groups):
        grid = max(groups[name])
        v = groups[name][grid]
        short = re.sub(r"mgk::|mgcv::|mgkv::|__attribute__\(\(ext_vector_type\(2\)\)\)|void ", "", name)
        print(f"calls {len(v):5d}  grid {grid:9d}  median {np.median(v):8.1f} us  min {min(v):8.1f}  max {max(v):8.1f}  {short[:150]}")


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
