"""Blocks of right-hand sides on K-cycle / Jac-GMRES complex hierarchies (``blockKcycle=True``) against the only route there was
before - the columns one after the other through the vector form - on the problem of profiles/complex_kcycle_measure.py: shifted
Laplacian at 128^3 cells (k h = 0.25, damping 0.5, four levels, omega 0.8), system operator with damping 0.05, ComplexF64 and
ComplexF32.  The numbers of profiles/complex_kcycle_blocks.md.
    python profiles/complex_kcycle_blocks_measure.py all [out.json]      ms per cycle AND COLUMN of V(2,1) Jac-GMRES, K(2,1) Jac and
                                                                         K(2,1) Jac-GMRES on blocks of 2 / 4 / 8 / 16 columns and on one
                                                                         vector (one warm-up, then 5 rounds; schedules, widths and
                                                                         precisions alternate inside every round); one block
                                                                         FGMRES(10) run to 1e-8 with the K(2,1) Jac cycle at 4 and 8
                                                                         columns against that many runs of the vector driver
    python profiles/complex_kcycle_blocks_measure.py regress OTHER_ROOT [out.json]
                                                                         the paths the change leaves alone, THIS tree against another
                                                                         built tree (the parent commit), one child process each, rounds
                                                                         alternating: the ComplexF64 V(2,1) Jac cycle, its 4-column
                                                                         block cycle (the z1-capable RESID) and the vector K(2,1)
                                                                         Jac-GMRES cycle - ms per cycle and a digest of the result
    python profiles/complex_kcycle_blocks_measure.py trace               the run to put under rocprofv3 --kernel-trace --output-format
                                                                         csv: per precision, 5 relaxations of 3 directions on the fine
                                                                         level for one vector and for 2 / 4 / 8 / 16 columns, then 5
                                                                         V(2,1) Jac block cycles per width
    python profiles/complex_kcycle_blocks_measure.py stats <kernel_trace.csv>
                                                                         the fine-level launches of that run in launch order: the GRAM
                                                                         step j = 0, 1, 2 per width and the block SMOOTH sweep per
                                                                         width - median, min - max in us, per column, and the byte model
Times of `all` and `regress` are wall-clock around CYCLES cycles between device synchronisations (a Jac-GMRES / K cycle synchronises
the host itself, so its host time is part of what it costs).  CK_CELLS overrides the 128 (rehearsals)."""
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
REPS, WARM, CYCLES = 5, 1, 5
TOL, MAXIT = 1e-8, 200
WIDTHS = (2, 4, 8, 16)
SCHEDULES = [("Jac-GMRES", "V"), ("Jac", "K"), ("Jac-GMRES", "K")]
TRACE_CALLS, TRACE_INNER = 5, 3


def build(mg, single, flag=True, relax="Jac", cyc="V"):
    from complex_cases import helmholtz
    Ah, mesh = helmholtz(mg, [CELLS] * 3, 0.25, 0.5)
    kw = {}
    if single:
        kw.update(singlePrecision=True, singleKcycle=True)
    if flag:
        kw.update(blockKcycle=True)
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


def blocks(torch, n, widths=WIDTHS):
    from complex_cases import complex_rhs
    out = {}
    for k in widths:
        B = torch.from_numpy(np.ascontiguousarray(np.stack([complex_rhs(n, 40 + j) for j in range(k)], axis=1))).cuda()
        out[k] = (B, torch.zeros_like(B))
    return out


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
    blk = blocks(torch, n)
    out = dict(cells=CELLS, n=n, nnz=int(As.nnz), cycles=CYCLES, reps=REPS, hbm_mib={}, cycle_ms_per_column={}, krylov={})
    devs = {}
    for prec in ("CF64", "CF32"):
        p = build(mg, prec == "CF32", relax="Jac-GMRES", cyc="K")
        dev = mg.device.DeviceHierarchy(p)
        dev.cycle_dev(bt, xt, 1)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        dev.block_cycle_dev(*blk[16], 1)
        torch.cuda.synchronize()
        out["hbm_mib"][prec + " block work set of 16 columns, K(2,1) Jac-GMRES (level blocks, staging, directions)"] = \
            (free0 - torch.cuda.mem_get_info()[0]) / 2 ** 20
        devs[prec] = (p, dev)
    print("hbm", json.dumps(out["hbm_mib"]), flush=True)
    keys = [(prec, s, k) for s in SCHEDULES for k in (1,) + WIDTHS for prec in ("CF64", "CF32")]
    t = {key: [] for key in keys}
    for rep in range(WARM + REPS):                               # schedules, widths and precisions alternate inside every round
        for prec, s, k in keys:
            p, dev = devs[prec]
            switch(p, dev, *s)
            if k == 1:                                           # the vector form: what a column cost before, one after the other
                run = lambda: dev.cycle_dev(bt, xt, 1)
            else:
                run = lambda: dev.block_cycle_dev(blk[k][0], blk[k][1], 1)
            run()                                                # (the first cycle behind a schedule change is not timed)
            sec = timed(torch, lambda: [run() for _ in range(CYCLES)])[0]
            if rep >= WARM:
                t[(prec, s, k)].append(1e3 * sec / CYCLES / k)
    for prec, s, k in keys:
        name = "%s %s %s(2,1) k=%d" % (prec, s[0], s[1], k)
        out["cycle_ms_per_column"][name] = stat(t[(prec, s, k)])
        print("cycle", name, json.dumps(out["cycle_ms_per_column"][name]), flush=True)
    # block FGMRES(10) with the K(2,1) Jac cycle against k runs of the vector driver
    for prec in ("CF64", "CF32"):
        p, dev = devs[prec]
        switch(p, dev, "Jac", "K")
        dev.set_krylov_operator(As)
        rec = {}
        runs = []
        for rep in range(WARM + 3):
            xt.zero_()
            sec, (flag, it, rv) = timed(torch, lambda: dev.fgmres_dev(bt, xt, 10, TOL, MAXIT))
            if rep >= WARM:
                runs.append(sec)
        x = xt.cpu().numpy()
        rec["vector"] = dict(flag=flag, steps=it, seconds=stat(runs), ms_per_step=1e3 * float(np.median(runs)) / max(it, 1),
                             true_residual=float(np.linalg.norm(b - As @ x) / np.linalg.norm(b)))
        for k in (4, 8):
            B, X = blk[k]
            runs = []
            for rep in range(WARM + 3):
                X.zero_()
                sec, (flag, it, rv) = timed(torch, lambda: dev.block_fgmres_dev_CFP64(B, X, 10, TOL, MAXIT))
                if rep >= WARM:
                    runs.append(sec)
            Bh, Xh = B.cpu().numpy(), X.cpu().numpy()
            rec["block k=%d" % k] = dict(flag=flag, steps=it, seconds=stat(runs), ms_per_step=1e3 * float(np.median(runs)) / max(it, 1),
                                         ms_per_step_and_column=1e3 * float(np.median(runs)) / max(it, 1) / k,
                                         seconds_per_column=float(np.median(runs)) / k,
                                         true_residual=float(np.linalg.norm(Bh - As @ Xh) / np.linalg.norm(Bh)))
        out["krylov"][prec + " FGMRES(10), K(2,1) Jac"] = rec
        print("krylov", prec, json.dumps(rec), flush=True)
    for p, dev in devs.values():
        dev.close()
    if out_path:
        json.dump(out, open(out_path, "w"), indent=1)


def child():
    """One tree's ComplexF64 hierarchy (no flag: the other tree may not know it); a line on stdin names what to time."""
    import torch
    import multigrid_jl_amd as mg
    from complex_cases import complex_rhs
    pd = build(mg, False, flag=False)
    dd = mg.device.DeviceHierarchy(pd)
    n = pd.As[0].shape[0]
    bt = torch.from_numpy(complex_rhs(n, 21)).cuda()
    xt = torch.zeros_like(bt)
    Bt, Xt = blocks(torch, n, (4,))[4]
    digest = lambda a: hashlib.sha1(a.cpu().numpy().tobytes()).hexdigest()[:16]
    print("ready", flush=True)
    for line in sys.stdin:
        what = line.strip()
        if what in ("cf64_v_jac", "cf64_k_jacgmres"):
            switch(pd, dd, *(("Jac", "V") if what == "cf64_v_jac" else ("Jac-GMRES", "K")))
            dd.cycle_dev(bt, xt, 1)
            sec = timed(torch, lambda: [dd.cycle_dev(bt, xt, 1) for _ in range(2 * CYCLES)])[0]
            res = xt
        elif what == "cf64_block4":
            switch(pd, dd, "Jac", "V")
            dd.block_cycle_dev(Bt, Xt, 1)
            sec = timed(torch, lambda: [dd.block_cycle_dev(Bt, Xt, 1) for _ in range(2 * CYCLES)])[0]
            res = Xt
        else:
            break
        print(1e3 * sec / (2 * CYCLES), digest(res), flush=True)
    dd.close()


WHATS = ("cf64_v_jac", "cf64_block4", "cf64_k_jacgmres")


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
        out["same bits " + what] = bool(bits[what]["this"] == bits[what]["other"] and len(bits[what]["this"]) == 1)
    for key, v in out.items():
        print(key, json.dumps(v), flush=True)
    if out_path:
        json.dump(out, open(out_path, "w"), indent=1)


def trace():
    """A fixed launch order, so that `stats` can tell the launches apart by their position."""
    import torch
    import multigrid_jl_amd as mg
    from complex_cases import complex_rhs
    for single in (False, True):
        p = build(mg, single, relax="Jac-GMRES", cyc="V")
        dev = mg.device.DeviceHierarchy(p)
        n = p.As[0].shape[0]
        cd = np.complex64 if single else np.complex128
        r0, x = complex_rhs(n, 21).astype(cd), np.zeros(n, dtype=cd)
        for _ in range(TRACE_CALLS):
            dev.fgmres_relax(1, r0, x, TRACE_INNER)
        for k in WIDTHS:
            R0 = np.asfortranarray(np.stack([complex_rhs(n, 40 + j) for j in range(k)], axis=1))
            X = np.zeros_like(R0)
            for _ in range(TRACE_CALLS):
                dev.block_fgmres_relax(1, R0, X, TRACE_INNER)
        switch(p, dev, "Jac", "V")
        for k, (B, X) in blocks(torch, n).items():
            for _ in range(TRACE_CALLS):
                dev.block_cycle_dev(B, X, 1)
        torch.cuda.synchronize()
        print("traced", "CF32" if single else "CF64", flush=True)
        dev.close()


def stats(path):
    """Template argument 1 of cx_csr_stream_spmv / cx_csr_stream_spmm: 0 AXPBY, 1 RESID, 2 SMOOTH, 3 GRAM; the last argument is the pair
    type.  The fine level is the largest grid of a kernel; within it the launches come in trace()'s order."""
    rows = []
    for r in csv.DictReader(open(path)):
        name = r.get("Kernel_Name") or r.get("Name") or ""
        m = re.search(r"cx_csr_stream_(spmv|spmm)<\(?(?:int\))?(\d)", name)
        if not m:
            continue
        prec = "CF32" if re.search(r"float", name.split("cx_csr_stream_")[1]) else "CF64"
        grid = int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)
        rows.append((float(r["Start_Timestamp"]), m.group(1), int(m.group(2)), prec, grid,
                     (float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    fine = max(g for _, _, _, _, g, _ in rows)
    N1 = CELLS + 1
    n, nnz = N1 ** 3, 7 * N1 ** 3 - 6 * N1 ** 2                  # the 7-point operator on the nodal grid
    for prec in ("CF64", "CF32"):
        vb = 16 if prec == "CF64" else 8
        sel = lambda kern, mode: [d for _, kk, mm, pp, g, d in rows if (kk, mm, pp, g) == (kern, mode, prec, fine)]
        v = sel("spmv", 3)
        assert len(v) == TRACE_CALLS * TRACE_INNER, (prec, len(v))
        for j in range(TRACE_INNER):
            d = v[j::TRACE_INNER]
            print(f"{prec} vector GRAM step j={j}: median {np.median(d):8.1f} us  min {min(d):8.1f}  max {max(d):8.1f}")
        g = sel("spmm", 3)
        assert len(g) == len(WIDTHS) * TRACE_CALLS * TRACE_INNER, (prec, len(g))
        s = sel("spmm", 2)
        per = len(s) // len(WIDTHS)
        for i, k in enumerate(WIDTHS):
            gk = g[i * TRACE_CALLS * TRACE_INNER:(i + 1) * TRACE_CALLS * TRACE_INNER]
            for j in range(TRACE_INNER):
                d = gk[j::TRACE_INNER]
                # bytes per row and column: the matrix stream / k (nnz / n entries of vb + 4 bytes, a row pointer, d[row] where znext is
                # written), the gather of Z_j, W and znext written, R0, and j earlier blocks of AZ read
                znext = 1 if j + 1 < TRACE_INNER else 0
                model = (nnz / n * (vb + 4) + 4 + vb * znext) / k + vb * (1 + 1 + znext + 1 + j)
                med = float(np.median(d))
                print(f"{prec} block GRAM k={k:2d} j={j}: median {med:8.1f} us  min {min(d):8.1f}  max {max(d):8.1f}   per column "
                      f"{med / k:7.1f} us   model {model:6.1f} B per row and column -> {model * n * k / med / 1e6:6.2f} TB/s")
            sk = s[i * per:(i + 1) * per]
            smodel = (nnz / n * (vb + 4) + 4 + vb) / k + 3 * vb     # (the block SMOOTH sweep: the stream and d / k, X gathered, B, X out)
            print(f"{prec} block SMOOTH k={k:2d}: {len(sk)} launches, median {np.median(sk):8.1f} us  min {min(sk):8.1f}  max {max(sk):8.1f}   "
                  f"per column {np.median(sk) / k:7.1f} us   model {smodel:6.1f} B per row and column -> "
                  f"{smodel * n * k / np.median(sk) / 1e6:6.2f} TB/s")


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
