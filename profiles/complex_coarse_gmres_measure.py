"""The GMRES coarsest solve of complex hierarchies on the device (coarseSolveType "GMRES"): what profiles/complex_coarse_gmres.md reports.
    python profiles/complex_coarse_gmres_measure.py all [out.json]
        counts    launches of one coarsest solve on both paths (mg_coarse_form) against the budget
        solve     the coarsest solve alone on shifted-Laplacian levels of 5^3, 9^3, 17^3 and 33^3 rows (hierarchies of one level, so a
                  cycle IS the solve): the one-workgroup tail, the chain of passes, and the dense inverse / sparse LU of the same operator
        cycle     128^3 cells, four levels, V(2,1) Jac: ms per cycle with the GMRES and with the dense-inverse coarsest solve, and
                  FGMRES(10) to 1e-8 on the operator with damping 0.05 with each as preconditioner: steps, flag, seconds
        resetup   replaceMatrixInHierarchy plus the first following cycle at 128^3, four levels, SPAI: GMRES against the LU path
    python profiles/complex_coarse_gmres_measure.py regress OTHER_LIB [out.json]
        what exists: the V(2,1) Jac cycle with the dense inverse and the 4-column block cycle of THIS tree's library against another
        build of libmgvcycle.so (the parent commit's), one child process each, rounds alternating between the two
    python profiles/complex_coarse_gmres_measure.py rehearse
        everything the above builds on the host, at 16^3 cells, without a device
Times are wall-clock around a batch of calls between device synchronisations, medians of REPS rounds in which the variants alternate,
with min and max as the spread (a GMRES coarsest solve synchronises the host itself: its host time is part of what it costs).
CG_CELLS overrides the 128 (rehearsals)."""
import copy
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CELLS = int(os.environ.get("CG_CELLS", "128"))
REPS, WARM = 5, 1
NEW_SYMBOLS = ("mg_set_coarse_gmres_CF64", "mg_coarse_gmres_CF64")


def stat(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def one_level_param(mg, A, coarse):
    from multigrid_jl_amd.mgsetup import defineCoarsestAinv
    p = mg.getMGparam(np.complex128, np.int64, 1, 8, 4, 1e-10, "Jac", 0.8, 1, 1, "V", coarse)
    p.As, p.Ps, p.Rs, p.relaxPrecs = [A], [], [], []
    p.nrhs = 1
    defineCoarsestAinv(p, A)
    return p


def hierarchy(mg, relax, coarse, cells=None):
    from complex_cases import helmholtz
    Ah, mesh = helmholtz(mg, [cells or CELLS] * 3, 0.25, 0.5)
    p = mg.getMGparam(np.complex128, np.int64, 4, 8, 200, 1e-8, relax, 0.8 if relax == "Jac" else 1.0, 2, 1, "V", coarse, 0.5, 0.0)
    mg.MGsetup(Ah, mesh, p)
    return p, Ah, mesh


def with_gmres_coarse(p):
    """The same hierarchy with the coarsest solve switched to GMRES (nothing of `p` is modified)."""
    from multigrid_jl_amd.mgsetup import defineCoarsestAinv
    q = copy.copy(p)
    q.coarseSolveType, q.LU, q.device = "GMRES", None, None
    defineCoarsestAinv(q, q.As[-1])
    return q


def set_path(dev, rows):
    assert dev.lib.mg_set_option(dev.handle, b"coarse_gmres_tail_rows", float(rows)) == 0


# ---- solve alone -----------------------------------------------------------------------------------------------------------------------
def measure_solve(mg, torch, out, sizes=(4, 8, 16, 32)):
    from complex_cases import complex_rhs, helmholtz
    out["counts"], out["solve_us"] = {}, {}
    for c in sizes:
        A, _ = helmholtz(mg, [c] * 3, 0.25, 0.5)
        n = A.shape[0]
        bt = torch.from_numpy(complex_rhs(n, 31)).cuda()
        xt = torch.zeros(n, dtype=torch.complex128, device="cuda")
        t0 = time.perf_counter()
        devs = {"gmres": mg.device.DeviceHierarchy(one_level_param(mg, A, "GMRES")), "factors": mg.device.DeviceHierarchy(one_level_param(mg, A, "NoMUMPS"))}
        host_s = time.perf_counter() - t0
        variants = [("chain", "gmres", 0)] + ([("tail", "gmres", -1)] if n <= 8192 else []) + [("factors", "factors", None)]
        counts = {}
        for name, d, rows in variants:
            if rows is not None:
                set_path(devs[d], rows)
            counts[name] = devs[d].coarse_form()
        batch = 200 if n < 10000 else 50
        t = {v[0]: [] for v in variants}
        for rep in range(WARM + REPS):
            for name, d, rows in variants:
                if rows is not None:
                    set_path(devs[d], rows)
                sec = timed(torch, lambda: [devs[d].cycle_dev(bt, xt, 1) for _ in range(batch)])[0]
                if rep >= WARM:
                    t[name].append(1e6 * sec / batch)
        out["counts"][str(n)] = counts
        out["solve_us"][str(n)] = {k: stat(v) for k, v in t.items()}
        print(f"n_c = {n}: " + "  ".join(f"{k} {np.median(v):.1f} us [{min(v):.1f}, {max(v):.1f}] ({counts[k]['launches']} launches, kind {counts[k]['kind']})"
                                         for k, v in t.items()) + f"   (host set-up of both handles {host_s:.2f} s)", flush=True)
        for dv in devs.values():
            dv.close()


# ---- cycle and FGMRES at 128^3 ---------------------------------------------------------------------------------------------------------
def measure_cycle(mg, torch, out):
    from complex_cases import complex_rhs, helmholtz
    t0 = time.perf_counter()
    pd, Ah, mesh = hierarchy(mg, "Jac", "NoMUMPS")
    t_setup = time.perf_counter() - t0
    pg = with_gmres_coarse(pd)
    As, _ = helmholtz(mg, [CELLS] * 3, 0.25, 0.05)
    n = As.shape[0]
    b = complex_rhs(n, 21)
    bt = torch.from_numpy(b).cuda()
    xt = torch.zeros(n, dtype=torch.complex128, device="cuda")
    t0 = time.perf_counter()
    devs = {"dense inverse": mg.device.DeviceHierarchy(pd)}
    t_dense = time.perf_counter() - t0
    t0 = time.perf_counter()
    devs["GMRES"] = mg.device.DeviceHierarchy(pg)
    t_gm = time.perf_counter() - t0
    print(f"{CELLS}^3: host MGsetup {t_setup:.1f} s, upload with the dense inverse {t_dense:.2f} s, with GMRES {t_gm:.2f} s; coarsest rows {pd.As[-1].shape[0]}",
          flush=True)
    CYC = 10
    t = {k: [] for k in devs}
    for rep in range(WARM + REPS):
        for k, dev in devs.items():
            sec = timed(torch, lambda: [dev.cycle_dev(bt, xt, 1) for _ in range(CYC)])[0]
            if rep >= WARM:
                t[k].append(1e3 * sec / CYC)
    out["cycle_ms"] = {k: stat(v) for k, v in t.items()}
    out["cycle_upload_s"] = {"dense inverse": t_dense, "GMRES": t_gm}
    out["fgmres10"] = {}
    for k, dev in devs.items():
        dev.set_krylov_operator(As)
        x = np.zeros_like(b)
        sec, r = timed(torch, lambda: dev.fgmres(b, x, 10, 1e-8, 200))
        res = float(np.linalg.norm(b - As @ x) / np.linalg.norm(b))
        out["fgmres10"][k] = dict(steps=int(r[2]), flag=int(r[1]), seconds=sec, true_residual=res)
        print(f"  {k}: cycle {np.median(t[k]):.3f} ms [{min(t[k]):.3f}, {max(t[k]):.3f}]; FGMRES(10) {r[2]} steps, flag {r[1]}, {sec:.3f} s, true residual {res:.2e}",
              flush=True)
    for dev in devs.values():
        dev.close()


# ---- re-setup --------------------------------------------------------------------------------------------------------------------------
def measure_resetup(mg, torch, out):
    from complex_cases import complex_rhs, helmholtz
    out["resetup_s"] = {}
    A2, _ = helmholtz(mg, [CELLS] * 3, 0.25, 0.35)
    for coarse in ("GMRES", "NoMUMPS"):
        p, Ah, mesh = hierarchy(mg, "SPAI", coarse)
        b = complex_rhs(Ah.shape[0], 21)
        x = np.zeros_like(b)
        mg.recursiveCycle(p, b, x, 1)                      # resident
        dev = p.device
        ts = []
        for rep in range(3):
            x[...] = 0
            sec = timed(torch, lambda: (mg.replaceMatrixInHierarchy(p, A2 if rep % 2 == 0 else Ah), mg.recursiveCycle(p, b, x, 1)))[0]
            assert p.device is dev
            ts.append(sec)
        out["resetup_s"][coarse] = stat(ts)
        print(f"  re-setup + first cycle, SPAI, coarsest solve {coarse}: {np.median(ts):.3f} s [{min(ts):.3f}, {max(ts):.3f}]", flush=True)
        mg.clear_(p)


# ---- what exists, against another build --------------------------------------------------------------------------------------------------
def child():
    """One process on the library named by MGVCYCLE_LIB: rounds are driven over stdin-free files by the parent - here simply REPS
    rounds of both cycles, printed as JSON."""
    import torch
    import multigrid_jl_amd as mg
    if os.environ.get("CG_OTHER") == "1":
        for k in NEW_SYMBOLS:
            mg.device.SIGNATURES.pop(k, None)
    from complex_cases import complex_rhs
    p, Ah, mesh = hierarchy(mg, "Jac", "NoMUMPS")
    n = Ah.shape[0]
    dev = mg.device.DeviceHierarchy(p)
    b = complex_rhs(n, 21)
    bt = torch.from_numpy(b).cuda()
    xt = torch.zeros(n, dtype=torch.complex128, device="cuda")
    Bt = torch.stack([bt, 2 * bt, 3 * bt, 4 * bt], dim=1).contiguous()
    Xt = torch.zeros_like(Bt)
    tv, tb = [], []
    for rep in range(WARM + REPS):
        s1 = timed(torch, lambda: [dev.cycle_dev(bt, xt, 1) for _ in range(10)])[0]
        s2 = timed(torch, lambda: [dev.block_cycle_dev(Bt, Xt, 1) for _ in range(5)])[0]
        if rep >= WARM:
            tv.append(1e3 * s1 / 10)
            tb.append(1e3 * s2 / 5)
    print("RESULT " + json.dumps(dict(vcycle_ms=tv, block4_ms=tb, x_sum=float(abs(xt.cpu().numpy()).sum()))), flush=True)
    dev.close()


def regress(other_lib, out_path):
    """Three child processes per library, alternating: this, other, this, other, ..."""
    res = {"this": dict(vcycle_ms=[], block4_ms=[]), "other": dict(vcycle_ms=[], block4_ms=[])}
    sums = {}
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
            for k in ("vcycle_ms", "block4_ms"):
                res[which][k] += r[k]
            sums[which] = r["x_sum"]
    out = {w: {k: stat(v) for k, v in d.items()} for w, d in res.items()}
    out["same_bits"] = sums["this"] == sums["other"]
    for k in ("vcycle_ms", "block4_ms"):
        print(f"{k}: this {out['this'][k]['median']:.3f} [{out['this'][k]['min']:.3f}, {out['this'][k]['max']:.3f}]   "
              f"other {out['other'][k]['median']:.3f} [{out['other'][k]['min']:.3f}, {out['other'][k]['max']:.3f}]")
    print("same sum of |x|:", out["same_bits"])
    if out_path:
        json.dump(out, open(out_path, "w"), indent=1)


def rehearse():
    import multigrid_jl_amd as mg
    from complex_cases import helmholtz
    for c in (4, 8):
        A, _ = helmholtz(mg, [c] * 3, 0.25, 0.5)
        for coarse in ("GMRES", "NoMUMPS"):
            p = one_level_param(mg, A, coarse)
            print(c, coarse, type(p.LU).__name__, A.shape)
    pd, Ah, mesh = hierarchy(mg, "Jac", "NoMUMPS", 16)
    pg = with_gmres_coarse(pd)
    print("levels", [M.shape[0] for M in pd.As], type(pd.LU).__name__, type(pg.LU).__name__, pg.coarseSolveType, pd.coarseSolveType)
    ps, _, _ = hierarchy(mg, "SPAI", "GMRES", 16)
    print("SPAI GMRES", ps.LU.shape)


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
