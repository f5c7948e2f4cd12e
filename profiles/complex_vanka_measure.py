"""The Vanka cell-block smoother in the complex cycle (getMGparam(np.complex128, ..., complexVanka=True)): what
profiles/complex_vanka.md reports.
    python profiles/complex_vanka_measure.py all [out.json]
        cycles    the mixed 3-D operator of tests/vanka_cases.py on CV_CELLS^3 cells (damping 0.1, omega CV_OMEGA), four levels,
                  VankaFaces, w = 0.6: ms per cycle from zero of the CF64 V(1,1) and K(1,1) cycles, the CF32 V(1,1) cycle and the
                  FP64 V(1,1) cycle on the real operator of the same grid, with the bytes each hierarchy holds in HBM
        fgmres    one FGMRES(5) inner step (one restart of 5 steps / 5) with the CF64 and the CF32 hierarchy as preconditioner
        zero      the cycle from zero with the from-zero mode (x_is_zero = 1) against the general path of the same library
                  (x_is_zero = 0 on a zero x), VankaFaces and VankaFacesAdd, CF64 and CF32; the results are compared bit for bit
    python profiles/complex_vanka_measure.py regress OTHER_LIB [out.json]
        what exists, THIS tree's library against another build of libmgvcycle.so (the parent commit's), one child process each,
        rounds alternating: the FP64 Vanka V(1,1) cycle, the ComplexF64 V(2,1) Jac cycle and the 4-column block cycle; the bits
        of their results are compared
    python profiles/complex_vanka_measure.py rehearse
        everything the above builds on the host, at 16^3 cells, without a device
Times are wall-clock around a batch of cycles on device vectors between two device synchronisations, medians of REPS rounds in
which the variants alternate, with min and max as the spread."""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CELLS = int(os.environ.get("CV_CELLS", "64"))
OMEGA = float(os.environ.get("CV_OMEGA", "0.15"))
REPS, WARM, BATCH = 5, 1, 10
NEW_SYMBOLS = ("mg_set_vanka_CF64", "mg_set_vanka_CF32", "mg_set_vanka_relax_CF64", "mg_set_vanka_relax_CF32")
MIXED = "SystemsFacesMixedLinear"


def stat(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def fmt(s):
    return f"{s['median']:.3f} [{s['min']:.3f}, {s['max']:.3f}]"


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def vanka_param(mg, A, cells, VAL, relaxType="VankaFaces", cycle="V", single=False, levels=4):
    kw = dict(singlePrecision=single, complexVanka=True) if np.dtype(VAL) == np.complex128 else {}
    p = mg.getMGparam(VAL, np.int64, levels, 1, 1, 1e-8, relaxType, 0.6, 1, 1, cycle, "NoMUMPS", 0.4, 0.0, MIXED, **kw)
    mg.MGsetup(A, mg.getRegularMesh([0, 1] * 3, [cells] * 3), p)
    return p


def retyped(mg, p, relaxType=None, cycle=None):
    """The hierarchy of `p` with another cycle type, or with the blocks of another Vanka type: the operators are shared."""
    import copy
    q = copy.copy(p)
    q.device = None
    if cycle:
        q.cycleType = cycle
    if relaxType:
        q.relaxType = relaxType
        q.relaxPrecs = [mg.getRelaxPrec(q.As[l], relaxType, 0.6, q.Meshes[l], True) for l in range(q.levels - 1)]
    return q


def hbm_bytes(p):
    """Bytes the hierarchy holds in HBM: operator values and int32 indices, the blocks, the pointwise slot."""
    tot = 0
    for M in list(p.As) + list(p.Ps) + list(p.Rs):
        tot += M.data.nbytes + 4 * M.nnz + 4 * (M.shape[0] + 1)
    for D in p.relaxPrecs:
        tot += D.nbytes
    return tot


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def device_pair(torch, b):
    bt = torch.from_numpy(np.ascontiguousarray(b, dtype=np.complex128)).cuda()
    return bt, torch.zeros_like(bt)


def rounds(torch, variants):
    """variants: name -> callable that enqueues one cycle; alternating rounds of BATCH cycles each.  ms per cycle."""
    t = {k: [] for k in variants}
    for rep in range(WARM + REPS):
        for k, fn in variants.items():
            sec = timed(torch, lambda: [fn() for _ in range(BATCH)])[0]
            if rep >= WARM:
                t[k].append(1e3 * sec / BATCH)
    return {k: stat(v) for k, v in t.items()}


def measure(mg, torch, out, parts):
    import vanka_cases as V
    t0 = time.perf_counter()
    Ac = V.mixed_operator([CELLS] * 3, True, omega=OMEGA)
    Ar = V.mixed_operator([CELLS] * 3, True)
    n = Ac.shape[0]
    p64 = vanka_param(mg, Ac, CELLS, np.complex128)
    p32 = vanka_param(mg, Ac, CELLS, np.complex128, single=True)
    pr = vanka_param(mg, Ar, CELLS, np.float64)
    pk = retyped(mg, p64, cycle="K")
    out["setup_s"] = time.perf_counter() - t0
    out["unknowns"], out["nnz"], out["levels"] = n, int(Ac.nnz), [int(M.shape[0]) for M in p64.As]
    out["hbm_bytes"] = dict(cf64=hbm_bytes(p64), cf32=hbm_bytes(p32), fp64=hbm_bytes(pr))
    print(f"{CELLS}^3 cells: {n} unknowns, {Ac.nnz} non-zeros, levels {out['levels']}, host set-up of three hierarchies {out['setup_s']:.1f} s", flush=True)
    print("bytes in HBM: " + "  ".join(f"{k} {v / 1e6:.1f} MB" for k, v in out["hbm_bytes"].items()), flush=True)
    b = V.seeded(n, 5, cx=True)
    bt, xt = device_pair(torch, b)
    brt = torch.from_numpy(np.ascontiguousarray(b.real)).cuda()
    xrt = torch.zeros_like(brt)
    devs = {k: mg.device.DeviceHierarchy(q) for k, q in (("cf64_v", p64), ("cf64_k", pk), ("cf32_v", p32), ("fp64_v", pr))}
    if "cycles" in parts:
        variants = {"cf64_v": lambda: devs["cf64_v"].cycle_dev(bt, xt, 1), "cf64_k": lambda: devs["cf64_k"].cycle_dev(bt, xt, 1),
                    "cf32_v": lambda: devs["cf32_v"].cycle_dev(bt, xt, 1), "fp64_v": lambda: devs["fp64_v"].cycle_dev(brt, xrt, 1)}
        out["cycle_ms"] = rounds(torch, variants)
        for k, s in out["cycle_ms"].items():
            print(f"  cycle {k}: {fmt(s)} ms", flush=True)
    if "fgmres" in parts:
        out["fgmres_step_ms"] = {}
        t = {"cf64": [], "cf32": []}
        for rep in range(WARM + REPS):
            for k, d in (("cf64", devs["cf64_v"]), ("cf32", devs["cf32_v"])):
                xt.zero_()
                sec, r = timed(torch, lambda: d.fgmres_dev(bt, xt, 5, 1e-30, 1))
                steps = max(int(r[1]), 1)
                if rep >= WARM:
                    t[k].append(1e3 * sec / steps)
        out["fgmres_step_ms"] = {k: stat(v) for k, v in t.items()}
        for k, s in out["fgmres_step_ms"].items():
            print(f"  FGMRES(5) inner step, {k} hierarchy: {fmt(s)} ms", flush=True)
    for d in devs.values():
        d.close()
    if "zero" in parts:
        out["zero_ms"], out["zero_same_bits"] = {}, {}
        for single, base in ((False, p64), (True, p32)):
            for rt in ("VankaFaces", "VankaFacesAdd"):
                q = base if rt == "VankaFaces" else retyped(mg, base, relaxType=rt)
                q.device = None
                d = mg.device.DeviceHierarchy(q)
                key = f"{'cf32' if single else 'cf64'}_{rt}"
                res = {}
                if not single:
                    for name, xz in (("from_zero", 1), ("general", 0)):
                        xt.zero_()
                        d.cycle_dev(bt, xt, xz)
                        torch.cuda.synchronize()
                        res[name] = digest(xt.cpu().numpy())

                def general():
                    xt.zero_()
                    d.cycle_dev(bt, xt, 0)

                def from_zero():
                    xt.zero_()
                    d.cycle_dev(bt, xt, 1)
                if single:      # (the mixed closure of a CF32 handle runs from zero only: the host-pointer cycle takes x_is_zero = 0)
                    b32 = b.astype(np.complex64)
                    bits = {}
                    for name, xz in (("from_zero", 1), ("general", 0)):
                        x32 = np.zeros_like(b32)
                        d.cycle(b32, x32, xz)
                        bits[name] = digest(x32)
                    res = bits
                    variants = {"from_zero": lambda: d.cycle(b32, np.zeros_like(b32), 1), "general": lambda: d.cycle(b32, np.zeros_like(b32), 0)}
                else:
                    variants = {"from_zero": from_zero, "general": general}
                out["zero_ms"][key] = rounds(torch, variants)
                out["zero_same_bits"][key] = res["from_zero"] == res["general"]
                s = out["zero_ms"][key]
                print(f"  {key}: from zero {fmt(s['from_zero'])} ms, general path on a zero x {fmt(s['general'])} ms, same bits: {out['zero_same_bits'][key]}"
                      + ("   (host-pointer cycles: transfers included)" if single else ""), flush=True)
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
    pr = vanka_param(mg, V.mixed_operator([CELLS] * 3, True), CELLS, np.float64)
    Ah, mesh = helmholtz(mg, [CELLS] * 3, 0.25, 0.5)
    pj = mg.getMGparam(np.complex128, np.int64, 4, 8, 200, 1e-8, "Jac", 0.8, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(Ah, mesh, pj)
    dv, dj = mg.device.DeviceHierarchy(pr), mg.device.DeviceHierarchy(pj)
    br = torch.from_numpy(V.seeded(pr.As[0].shape[0], 5)).cuda()
    xr = torch.zeros_like(br)
    bj = torch.from_numpy(complex_rhs(Ah.shape[0], 21)).cuda()
    xj = torch.zeros_like(bj)
    Bj = torch.stack([bj, 2 * bj, 3 * bj, 4 * bj], dim=1).contiguous()
    Xj = torch.zeros_like(Bj)
    variants = {"fp64_vanka_v": lambda: dv.cycle_dev(br, xr, 1), "cf64_jac_v21": lambda: dj.cycle_dev(bj, xj, 1),
                "cf64_block4": lambda: dj.block_cycle_dev(Bj, Xj, 1)}
    t = {k: [] for k in variants}
    for rep in range(WARM + REPS):
        for k, fn in variants.items():
            sec = timed(torch, lambda: [fn() for _ in range(BATCH)])[0]
            if rep >= WARM:
                t[k].append(1e3 * sec / BATCH)
    bits = dict(fp64_vanka_v=digest(xr.cpu().numpy()), cf64_jac_v21=digest(xj.cpu().numpy()), cf64_block4=digest(Xj.cpu().numpy()))
    print("RESULT " + json.dumps(dict(ms=t, bits=bits)), flush=True)
    dv.close()
    dj.close()


def regress(other_lib, out_path):
    res = {"this": {}, "other": {}}
    bits = {}
    for rnd in range(2):
        for which in ("this", "other"):
            env = dict(os.environ)
            if which == "other":
                env["MGVCYCLE_LIB"], env["CV_OTHER"] = os.path.abspath(other_lib), "1"
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=500)
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-2000:])
                sys.exit(p.returncode)
            r = json.loads([ln for ln in p.stdout.split("\n") if ln.startswith("RESULT ")][0][7:])
            for k, v in r["ms"].items():
                res[which].setdefault(k, []).extend(v)
            bits[which] = r["bits"]
    out = {w: {k: stat(v) for k, v in d.items()} for w, d in res.items()}
    out["same_bits"] = {k: bits["this"][k] == bits["other"][k] for k in bits["this"]}
    out["cells"] = CELLS
    for k in res["this"]:
        print(f"{k}: this {fmt(out['this'][k])} ms   other {fmt(out['other'][k])} ms   same bits: {out['same_bits'][k]}", flush=True)
    if out_path:
        json.dump(out, open(out_path, "w"), indent=1)


def rehearse():
    import multigrid_jl_amd as mg
    import vanka_cases as V
    Ac = V.mixed_operator([16] * 3, True, omega=OMEGA)
    p64 = vanka_param(mg, Ac, 16, np.complex128, levels=2)
    p32 = vanka_param(mg, Ac, 16, np.complex128, single=True, levels=2)
    pa = retyped(mg, p32, relaxType="VankaFacesAdd")
    pk = retyped(mg, p64, cycle="K")
    print("levels", [M.shape[0] for M in p64.As], p64.relaxPrecs[0].dtype, p32.As[0].dtype, pa.relaxType, pk.cycleType,
          "bytes", hbm_bytes(p64), hbm_bytes(p32))


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
        out = dict(cells=CELLS, omega=OMEGA, reps=REPS, batch=BATCH)
        measure(mg, torch, out, sys.argv[3:] or ["cycles", "fgmres", "zero"])
        if len(sys.argv) > 2:
            json.dump(out, open(sys.argv[2], "w"), indent=1)
