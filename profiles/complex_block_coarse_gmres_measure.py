"""The block GMRES coarsest solve of complex hierarchies on the device (blockCoarseGMRES=True): what
profiles/complex_block_coarse_gmres.md reports.
    python profiles/complex_block_coarse_gmres_measure.py all [out.json] [parts...]
        solve     the block solve alone on shifted-Laplacian levels of 5^3, 9^3, 17^3 and 33^3 rows (hierarchies of one level, so a cycle
                  IS the solve) for 2 / 4 / 8 / 16 columns: the chain of passes, the one-workgroup form where n_c k <= 8192, against k
                  runs of the single-vector GMRES coarsest solve (the only route without the feature) and the explicit inverse applied
                  to the block (cx_dense_matblk; the sparse LU at 33^3)
        cycle     128^3 cells, four levels, V(2,1) Jac: ms per block cycle with the block GMRES coarsest solve and with the dense inverse,
                  against the single GMRES-coarse cycle; block FGMRES(10) to 1e-8 on the operator with damping 0.05, 4 columns
        resetup   replaceMatrixInHierarchy plus the first following block cycle (4 columns) at 128^3, four levels, SPAI: GMRES against LU
    python profiles/complex_block_coarse_gmres_measure.py regress OTHER_LIB [out.json]
        what exists: the V(2,1) Jac cycle with the dense inverse, its 4-column block cycle and the single-vector GMRES-coarse cycle of
        THIS tree's library against another build of libmgvcycle.so (the parent commit's), one child process each, alternating
    python profiles/complex_block_coarse_gmres_measure.py rehearse
        everything the above builds on the host, at small sizes, without a device
Times are wall-clock around a batch of calls between device synchronisations, medians of REPS rounds in which the variants alternate,
with min and max as the spread (a GMRES coarsest solve synchronises the host itself: its host time is part of what it costs).
CG_CELLS overrides the 128 (rehearsals)."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

from complex_coarse_gmres_measure import CELLS, REPS, WARM, hierarchy, one_level_param, set_path, stat, timed, with_gmres_coarse  # noqa: E402

NEW_SYMBOLS = ("mg_block_coarse_gmres_CF64", "mg_block_coarse_form")
KS = (2, 4, 8, 16)


def block_rhs(torch, n, k):
    from complex_cases import complex_rhs
    B = np.ascontiguousarray(np.stack([complex_rhs(n, 40 + j) for j in range(k)], axis=1))
    return torch.from_numpy(B).cuda()


# ---- solve alone -----------------------------------------------------------------------------------------------------------------------
def measure_solve(mg, torch, out, sizes=(4, 8, 16, 32)):
    from complex_cases import complex_rhs, helmholtz
    out["solve_us"], out["forms"] = {}, {}
    for c in sizes:
        A, _ = helmholtz(mg, [c] * 3, 0.25, 0.5)
        n = A.shape[0]
        pg = one_level_param(mg, A, "GMRES")
        pg.blockCoarseGMRES = True
        devs = {"gmres": mg.device.DeviceHierarchy(pg), "factors": mg.device.DeviceHierarchy(one_level_param(mg, A, "NoMUMPS"))}
        bt = torch.from_numpy(complex_rhs(n, 40)).cuda()
        xt = torch.zeros(n, dtype=torch.complex128, device="cuda")
        for k in KS:
            Bt, Xt = block_rhs(torch, n, k), torch.zeros((n, k), dtype=torch.complex128, device="cuda")
            variants = [("chain", "gmres", 0)] + ([("one workgroup", "gmres", 8192)] if n * k <= 8192 else []) + \
                       [("k single solves", "gmres", -1), ("factors", "factors", None)]
            batch = 100 if n < 10000 else 30
            t = {v[0]: [] for v in variants}
            forms = {}
            for rep in range(WARM + REPS):
                for name, d, rows in variants:
                    dev = devs[d]
                    if rows is not None:
                        set_path(dev, rows)
                    if name == "k single solves":
                        sec = timed(torch, lambda: [dev.cycle_dev(bt, xt, 1) for _ in range(batch * k)])[0]
                    else:
                        if d == "gmres":
                            forms[name] = dev.block_coarse_form(k)
                        sec = timed(torch, lambda: [dev.block_cycle_dev(Bt, Xt, 1) for _ in range(batch)])[0]
                    if rep >= WARM:
                        t[name].append(1e6 * sec / batch)
            set_path(devs["gmres"], -1)
            out["solve_us"][f"{n}x{k}"] = {kk: stat(v) for kk, v in t.items()}
            out["forms"][f"{n}x{k}"] = forms
            print(f"n_c = {n}, k = {k}: " + "  ".join(f"{kk} {np.median(v):.1f} us [{min(v):.1f}, {max(v):.1f}]" for kk, v in t.items())
                  + f"   factors kind {devs['factors'].coarse_form()['kind']}, launches {forms}", flush=True)
        for dv in devs.values():
            dv.close()


# ---- cycle and block FGMRES at 128^3 -----------------------------------------------------------------------------------------------------
def measure_cycle(mg, torch, out):
    from complex_cases import helmholtz
    t0 = time.perf_counter()
    pd, Ah, mesh = hierarchy(mg, "Jac", "NoMUMPS")
    t_setup = time.perf_counter() - t0
    pg = with_gmres_coarse(pd)
    pg.blockCoarseGMRES = True
    As, _ = helmholtz(mg, [CELLS] * 3, 0.25, 0.05)
    n = As.shape[0]
    devs = {"dense inverse": mg.device.DeviceHierarchy(pd), "block GMRES": mg.device.DeviceHierarchy(pg)}
    print(f"{CELLS}^3: host MGsetup {t_setup:.1f} s; coarsest rows {pd.As[-1].shape[0]}", flush=True)
    bt = block_rhs(torch, n, 1)[:, 0].contiguous()
    xt = torch.zeros(n, dtype=torch.complex128, device="cuda")
    CYC = 10
    out["cycle_ms_per_column"], out["cycle_forms"] = {}, {}
    ts = []
    for rep in range(WARM + REPS):
        sec = timed(torch, lambda: [devs["block GMRES"].cycle_dev(bt, xt, 1) for _ in range(CYC)])[0]
        if rep >= WARM:
            ts.append(1e3 * sec / CYC)
    out["cycle_ms_per_column"]["1 (single GMRES-coarse cycle)"] = stat(ts)
    print(f"  single GMRES-coarse cycle {np.median(ts):.3f} ms [{min(ts):.3f}, {max(ts):.3f}]", flush=True)
    for k in KS:
        Bt, Xt = block_rhs(torch, n, k), torch.zeros((n, k), dtype=torch.complex128, device="cuda")
        t = {kk: [] for kk in devs}
        for rep in range(WARM + REPS):
            for kk, dev in devs.items():
                sec = timed(torch, lambda: [dev.block_cycle_dev(Bt, Xt, 1) for _ in range(CYC)])[0]
                if rep >= WARM:
                    t[kk].append(1e3 * sec / CYC / k)
        out["cycle_ms_per_column"][str(k)] = {kk: stat(v) for kk, v in t.items()}
        out["cycle_forms"][str(k)] = devs["block GMRES"].block_coarse_form(k)
        print(f"  k = {k}: per column " + "  ".join(f"{kk} {np.median(v):.3f} ms [{min(v):.3f}, {max(v):.3f}]" for kk, v in t.items())
              + f"   {out['cycle_forms'][str(k)]}", flush=True)
    out["block_fgmres10"] = {}
    k = 4
    B = np.asfortranarray(block_rhs(torch, n, k).cpu().numpy())
    for kk, dev in devs.items():
        dev.set_krylov_operator(As)
        X = np.zeros_like(B)
        sec, r = timed(torch, lambda: dev.block_fgmres(B, X, 10, 1e-8, 200))
        res = float(np.linalg.norm(B - As @ X) / np.linalg.norm(B))
        out["block_fgmres10"][kk] = dict(steps=int(r[2]), flag=int(r[1]), seconds=sec, true_residual=res)
        print(f"  {kk}: block FGMRES(10), {k} columns: {r[2]} steps, flag {r[1]}, {sec:.3f} s, true residual {res:.2e}", flush=True)
    for dev in devs.values():
        dev.close()


# ---- re-setup --------------------------------------------------------------------------------------------------------------------------
def measure_resetup(mg, torch, out):
    from complex_cases import helmholtz
    out["resetup_s"] = {}
    A2, _ = helmholtz(mg, [CELLS] * 3, 0.25, 0.35)
    for coarse in ("GMRES", "NoMUMPS"):
        Ah, mesh = helmholtz(mg, [CELLS] * 3, 0.25, 0.5)
        kw = {"blockCoarseGMRES": True} if coarse == "GMRES" else {}
        p = mg.getMGparam(np.complex128, np.int64, 4, 8, 200, 1e-8, "SPAI", 1.0, 2, 1, "V", coarse, 0.5, 0.0, **kw)
        mg.MGsetup(Ah, mesh, p)
        B = np.asfortranarray(block_rhs(torch, Ah.shape[0], 4).cpu().numpy())
        X = np.zeros_like(B)
        mg.recursiveCycle(p, B, X, 1)                      # resident
        dev = p.device
        ts = []
        for rep in range(3):
            X[...] = 0
            sec = timed(torch, lambda: (mg.replaceMatrixInHierarchy(p, A2 if rep % 2 == 0 else Ah), mg.recursiveCycle(p, B, X, 1)))[0]
            assert p.device is dev
            ts.append(sec)
        out["resetup_s"][coarse] = stat(ts)
        print(f"  re-setup + first block cycle (4 columns), SPAI, coarsest solve {coarse}: {np.median(ts):.3f} s [{min(ts):.3f}, {max(ts):.3f}]", flush=True)
        mg.clear_(p)


# ---- what exists, against another build --------------------------------------------------------------------------------------------------
def child():
    import torch
    import multigrid_jl_amd as mg
    if os.environ.get("CG_OTHER") == "1":
        for k in NEW_SYMBOLS:
            mg.device.SIGNATURES.pop(k, None)
    pd, Ah, mesh = hierarchy(mg, "Jac", "NoMUMPS")
    pg = with_gmres_coarse(pd)
    n = Ah.shape[0]
    dev, devg = mg.device.DeviceHierarchy(pd), mg.device.DeviceHierarchy(pg)
    bt = block_rhs(torch, n, 1)[:, 0].contiguous()
    xt, xg = torch.zeros(n, dtype=torch.complex128, device="cuda"), torch.zeros(n, dtype=torch.complex128, device="cuda")
    Bt = torch.stack([bt, 2 * bt, 3 * bt, 4 * bt], dim=1).contiguous()
    Xt = torch.zeros_like(Bt)
    tv, tb, tg = [], [], []
    for rep in range(WARM + REPS):
        s1 = timed(torch, lambda: [dev.cycle_dev(bt, xt, 1) for _ in range(10)])[0]
        s2 = timed(torch, lambda: [dev.block_cycle_dev(Bt, Xt, 1) for _ in range(5)])[0]
        s3 = timed(torch, lambda: [devg.cycle_dev(bt, xg, 1) for _ in range(10)])[0]
        if rep >= WARM:
            tv.append(1e3 * s1 / 10)
            tb.append(1e3 * s2 / 5)
            tg.append(1e3 * s3 / 10)
    import hashlib
    bits = hashlib.sha256(xt.cpu().numpy().tobytes() + Xt.cpu().numpy().tobytes() + xg.cpu().numpy().tobytes()).hexdigest()
    print("RESULT " + json.dumps(dict(vcycle_ms=tv, block4_ms=tb, gmres_cycle_ms=tg, bits=bits)), flush=True)
    dev.close()
    devg.close()


def regress(other_lib, out_path):
    keys = ("vcycle_ms", "block4_ms", "gmres_cycle_ms")
    res = {w: {k: [] for k in keys} for w in ("this", "other")}
    bits = {}
    for rnd in range(2):
        for which in ("this", "other"):
            env = dict(os.environ)
            if which == "other":
                env["MGVCYCLE_LIB"], env["CG_OTHER"] = os.path.abspath(other_lib), "1"
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-2000:])
                sys.exit(p.returncode)
            r = json.loads([ln for ln in p.stdout.split("\n") if ln.startswith("RESULT ")][0][7:])
            for k in keys:
                res[which][k] += r[k]
            bits[which] = r["bits"]
    out = {w: {k: stat(v) for k, v in d.items()} for w, d in res.items()}
    out["same_bits"] = bits["this"] == bits["other"]
    for k in keys:
        print(f"{k}: this {out['this'][k]['median']:.3f} [{out['this'][k]['min']:.3f}, {out['this'][k]['max']:.3f}]   "
              f"other {out['other'][k]['median']:.3f} [{out['other'][k]['min']:.3f}, {out['other'][k]['max']:.3f}]", flush=True)
    print("same bits of all three results:", out["same_bits"], flush=True)
    if out_path:
        json.dump(out, open(out_path, "w"), indent=1)


def rehearse():
    import multigrid_jl_amd as mg
    from complex_cases import helmholtz
    A, _ = helmholtz(mg, [4] * 3, 0.25, 0.5)
    pg = one_level_param(mg, A, "GMRES")
    pg.blockCoarseGMRES = True
    print("one level", A.shape, type(pg.LU).__name__)
    pd, Ah, mesh = hierarchy(mg, "Jac", "NoMUMPS", 16)
    pg = with_gmres_coarse(pd)
    pg.blockCoarseGMRES = True
    print("levels", [M.shape[0] for M in pd.As], pg.coarseSolveType, pg.blockCoarseGMRES)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    if mode == "rehearse":
        rehearse()
    elif mode == "child":
        child()
    elif mode == "regress":
        regress(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        import torch
        import multigrid_jl_amd as mg
        out = dict(cells=CELLS, reps=REPS)
        parts = sys.argv[3:] or ["solve", "cycle", "resetup"]
        if "solve" in parts:
            measure_solve(mg, torch, out)
        if "cycle" in parts:
            measure_cycle(mg, torch, out)
        if "resetup" in parts:
            measure_resetup(mg, torch, out)
        if len(sys.argv) > 2:
            json.dump(out, open(sys.argv[2], "w"), indent=1)
