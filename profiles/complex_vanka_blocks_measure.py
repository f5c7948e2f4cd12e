"""Blocks of right-hand sides on complex Vanka hierarchies (getMGparam(..., complexVanka=True, vankaBlocks=True)): what
profiles/complex_vanka_blocks.md reports.  Problem and helpers: profiles/complex_vanka_measure.py (the mixed 3-D operator on
CV_CELLS^3 cells, damping 0.1, four levels, VankaFaces, w = 0.6).
    python profiles/complex_vanka_blocks_measure.py all [out.json] [parts]
        smoother  one VankaFaces iteration of the stand-alone smoother on the fine operator: the block pass at k = 1, 4, 16
                  (mg_vanka_time_block_dev) against the one-vector kernels (mg_vanka_time_dev), device events around every
                  iteration; the bits of the k = 4 block pass are compared with four one-vector passes
        cycles    the CF64 and the CF32 block V(1,1) cycle from zero at k = 4 and 16 against k single-vector cycles
        driver    one block-FGMRES(5) inner step at k = 16 (one restart of 5 steps / 5), CF64 and CF32 hierarchy
    python profiles/complex_vanka_blocks_measure.py regress OTHER_LIB [out.json]
        what exists, THIS tree's library against another build of libmgvcycle.so (the parent commit's), one child process each,
        rounds alternating: the FP64 Vanka V(1,1) cycle, the ComplexF64 one-vector Vanka V(1,1) cycle and the 4-column ComplexF64
        Jac block cycle; the bits of their results are compared
Cycle and driver times are wall clock around a batch on device blocks between two device synchronisations; all are medians of REPS
rounds in which the variants alternate, with min and max as the spread."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import complex_vanka_measure as M  # noqa: E402  (puts the repository root and tests/ on sys.path)

CELLS, OMEGA, REPS, WARM, BATCH = M.CELLS, M.OMEGA, M.REPS, M.WARM, M.BATCH
NEW_SYMBOLS = ("mg_vanka_apply_block_FP64", "mg_vanka_apply_block_dev_FP64", "mg_vanka_apply_block_CFP64",
               "mg_vanka_apply_block_dev_CFP64", "mg_vanka_time_block_dev")
KS = (1, 4, 16)


def flagged(mg, A, single=False):
    p = M.vanka_param(mg, A, CELLS, np.complex128, single=single)
    p.vankaBlocks = True
    return p


def seeded_block(torch, n, k):
    import vanka_cases as V
    B = np.stack([V.seeded(n, 5 + 7 * j, cx=True) for j in range(k)], axis=1)
    return torch.from_numpy(np.ascontiguousarray(B)).cuda()


def smoother(mg, torch, out, Ac):
    import vanka_cases as V
    lib = mg.device.load_library()
    nn = np.asarray([CELLS] * 3)
    D = mg.setupVankaFacesPreconditioner(Ac, nn, 0.6, True, V.FULL_VANKA_RB)
    n = Ac.shape[0]
    dp = C.POINTER(C.c_double)
    with mg.vanka.vanka_handle(Ac, D, nn, True) as H:
        # bits: the k = 4 block pass against four one-vector passes
        Bt, Xt = seeded_block(torch, n, 4), torch.zeros((n, 4), dtype=torch.complex128, device="cuda")
        H.apply_dev(Xt, Bt, 1, V.FULL_VANKA_RB)
        same = True
        for c in range(4):
            bc, xc = Bt[:, c].contiguous(), torch.zeros(n, dtype=torch.complex128, device="cuda")
            H.apply_dev(xc, bc, 1, V.FULL_VANKA_RB)
            same = same and bool(torch.equal(xc, Xt[:, c]))
        out["smoother_same_bits"] = same
        blocks = {k: (seeded_block(torch, n, k), torch.zeros((n, k), dtype=torch.complex128, device="cuda")) for k in KS}
        bv, xv = blocks[1][0][:, 0].contiguous(), torch.zeros(n, dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        t = {"one_vector": []}
        t.update({f"block_k{k}": [] for k in KS})
        ms = np.zeros(BATCH)
        for rep in range(WARM + REPS):
            mg.device._check(lib, lib.mg_vanka_time_dev(H.h, mg.device._ptr(xv), mg.device._ptr(bv), V.FULL_VANKA_RB, 1, BATCH,
                                                        ms.ctypes.data_as(dp)), "mg_vanka_time_dev")
            if rep >= WARM:
                t["one_vector"].append(float(np.median(ms)))
            for k in KS:
                Bk, Xk = blocks[k]
                mg.device._check(lib, lib.mg_vanka_time_block_dev(H.h, mg.device._ptr(Xk), mg.device._ptr(Bk), k, V.FULL_VANKA_RB, 1,
                                                                  BATCH, ms.ctypes.data_as(dp)), "mg_vanka_time_block_dev")
                if rep >= WARM:
                    t[f"block_k{k}"].append(float(np.median(ms)))
    out["smoother_ms"] = {k: M.stat(v) for k, v in t.items()}
    one = out["smoother_ms"]["one_vector"]["median"]
    out["smoother_per_column_ratio"] = {k: out["smoother_ms"][f"block_k{k}"]["median"] / (k * one) for k in KS}
    print(f"  smoother, one VankaFaces iteration: one vector {M.fmt(out['smoother_ms']['one_vector'])} ms; block bits = columns: {same}", flush=True)
    for k in KS:
        print(f"    block k={k}: {M.fmt(out['smoother_ms'][f'block_k{k}'])} ms, per column {out['smoother_per_column_ratio'][k]:.3f} of the one-vector pass",
              flush=True)


def measure(mg, torch, out, parts):
    import time
    import vanka_cases as V
    t0 = time.perf_counter()
    Ac = V.mixed_operator([CELLS] * 3, True, omega=OMEGA)
    n = Ac.shape[0]
    out["unknowns"] = n
    if "smoother" in parts:
        smoother(mg, torch, out, Ac)
    if not ({"cycles", "driver"} & set(parts)):
        return
    ps = {"cf64": flagged(mg, Ac), "cf32": flagged(mg, Ac, single=True)}
    out["setup_s"] = time.perf_counter() - t0
    devs = {k: mg.device.DeviceHierarchy(p) for k, p in ps.items()}
    bt, xt = M.device_pair(torch, V.seeded(n, 5, cx=True))
    if "cycles" in parts:
        out["cycle_ms"], out["cycle_per_column_ratio"] = {}, {}
        for k in (4, 16):
            Bt = seeded_block(torch, n, k)
            Xt = torch.zeros_like(Bt)
            variants = {}
            for name, d in devs.items():
                variants[f"{name}_block_k{k}"] = lambda d=d: d.block_cycle_dev(Bt, Xt, 1)
                variants[f"{name}_{k}_single_cycles"] = lambda d=d: [d.cycle_dev(bt, xt, 1) for _ in range(k)]
            r = M.rounds(torch, variants)
            out["cycle_ms"].update(r)
            for name in devs:
                ratio = r[f"{name}_block_k{k}"]["median"] / r[f"{name}_{k}_single_cycles"]["median"]
                out["cycle_per_column_ratio"][f"{name}_k{k}"] = ratio
                print(f"  {name} V(1,1) k={k}: block cycle {M.fmt(r[f'{name}_block_k{k}'])} ms, {k} single-vector cycles "
                      f"{M.fmt(r[f'{name}_{k}_single_cycles'])} ms, per column {ratio:.3f}", flush=True)
            del Bt, Xt
    if "driver" in parts:
        k = 16
        Bt = seeded_block(torch, n, k)
        Xt = torch.zeros_like(Bt)
        t = {name: [] for name in devs}
        for rep in range(WARM + REPS):
            for name, d in devs.items():
                Xt.zero_()
                sec, r = M.timed(torch, lambda: d.block_fgmres_dev_CFP64(Bt, Xt, 5, 1e-30, 1))
                if rep >= WARM:
                    t[name].append(1e3 * sec / max(int(r[1]), 1))
        out["block_fgmres_step_ms_k16"] = {name: M.stat(v) for name, v in t.items()}
        for name, s in out["block_fgmres_step_ms_k16"].items():
            print(f"  block FGMRES(5) inner step, k=16, {name} hierarchy: {M.fmt(s)} ms", flush=True)
    for d in devs.values():
        d.close()


# ---- what exists, against another build ----------------------------------------------------------------------------------------
def child():
    import torch
    import multigrid_jl_amd as mg
    if os.environ.get("CV_OTHER") == "1":
        for k in NEW_SYMBOLS:
            mg.device.SIGNATURES.pop(k, None)
    import vanka_cases as V
    from complex_cases import complex_rhs, helmholtz
    pr = M.vanka_param(mg, V.mixed_operator([CELLS] * 3, True), CELLS, np.float64)
    pc = M.vanka_param(mg, V.mixed_operator([CELLS] * 3, True, omega=OMEGA), CELLS, np.complex128)
    Ah, mesh = helmholtz(mg, [CELLS] * 3, 0.25, 0.5)
    pj = mg.getMGparam(np.complex128, np.int64, 4, 8, 200, 1e-8, "Jac", 0.8, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(Ah, mesh, pj)
    dv, dc, dj = (mg.device.DeviceHierarchy(q) for q in (pr, pc, pj))
    br = torch.from_numpy(V.seeded(pr.As[0].shape[0], 5)).cuda()
    xr = torch.zeros_like(br)
    bc, xc = M.device_pair(torch, V.seeded(pc.As[0].shape[0], 5, cx=True))
    bj = torch.from_numpy(complex_rhs(Ah.shape[0], 21)).cuda()
    Bj = torch.stack([bj, 2 * bj, 3 * bj, 4 * bj], dim=1).contiguous()
    Xj = torch.zeros_like(Bj)
    variants = {"fp64_vanka_v": lambda: dv.cycle_dev(br, xr, 1), "cf64_vanka_v": lambda: dc.cycle_dev(bc, xc, 1),
                "cf64_jac_block4": lambda: dj.block_cycle_dev(Bj, Xj, 1)}
    t = {k: [] for k in variants}
    for rep in range(WARM + REPS):
        for k, fn in variants.items():
            sec = M.timed(torch, lambda: [fn() for _ in range(BATCH)])[0]
            if rep >= WARM:
                t[k].append(1e3 * sec / BATCH)
    bits = dict(fp64_vanka_v=M.digest(xr.cpu().numpy()), cf64_vanka_v=M.digest(xc.cpu().numpy()), cf64_jac_block4=M.digest(Xj.cpu().numpy()))
    print("RESULT " + json.dumps(dict(ms=t, bits=bits)), flush=True)
    for d in (dv, dc, dj):
        d.close()


def regress(other_lib, out_path):
    res = {"this": {}, "other": {}}
    bits = {}
    for rnd in range(2):
        for which in ("this", "other"):
            env = dict(os.environ)
            if which == "other":
                env["MGVCYCLE_LIB"], env["CV_OTHER"] = os.path.abspath(other_lib), "1"
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=400)
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-2000:])
                sys.exit(p.returncode)
            r = json.loads([ln for ln in p.stdout.split("\n") if ln.startswith("RESULT ")][0][7:])
            for k, v in r["ms"].items():
                res[which].setdefault(k, []).extend(v)
            bits[which] = r["bits"]
    out = {w: {k: M.stat(v) for k, v in d.items()} for w, d in res.items()}
    out["same_bits"] = {k: bits["this"][k] == bits["other"][k] for k in bits["this"]}
    out["cells"] = CELLS
    for k in res["this"]:
        print(f"{k}: this {M.fmt(out['this'][k])} ms   other {M.fmt(out['other'][k])} ms   same bits: {out['same_bits'][k]}", flush=True)
    if out_path:
        json.dump(out, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    if mode == "child":
        child()
    elif mode == "regress":
        regress(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        import torch
        import multigrid_jl_amd as mg
        out = dict(cells=CELLS, omega=OMEGA, reps=REPS, batch=BATCH)
        measure(mg, torch, out, sys.argv[3:] or ["smoother", "cycles", "driver"])
        if len(sys.argv) > 2:
            json.dump(out, open(sys.argv[2], "w"), indent=1)
