"""Measurements behind profiles/parlu_single.md (single-precision factors in the device sparse-LU applier).
    python profiles/parlu_single_measure.py PART [--root TREE] [--out FILE.json]
PART:
  lu      mg_lu_time_dev on the 256 x 256-cell Helmholtz factor of profiles/parlu_complex.md: a ComplexF64 and a ComplexF32
          handle on the same factorisation (the single one rounded from it), nrhs 1 / 4 / 16, plain and adjoint, ROUNDS
          alternating rounds of REPS samples behind WARM warm-up solves; HBM each handle holds (free memory before and after
          its creation and after its adjoint set), the form each picked;
  cycle   the 2-level ComplexF32 hierarchy of profiles/coarse_solver.md on 512 x 512 cells with a ComplexF64 and with a
          ComplexF32 solver object as param.LU: ms per cycle, alternating, and FGMRES(20) step counts to 1e-8;
  parent  what the parent commit has too, for the unchanged-path check (--root names the tree whose package and built library
          are imported; run it on both trees, alternating): the ComplexF64 applier on the same factor, the ComplexF64
          V(2,1) Jac cycle at 64^3 cells and its 4-column block cycle - times and a SHA-256 of each result.
Applier times: events on the library's stream (mg_lu_time_dev).  Cycle times: host clock around CYCLES enqueued cycles ending
in a device synchronise, after a warm-up."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

import torch
import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("part", choices=["lu", "cycle", "parent"])
ap.add_argument("--root", default=HERE)
ap.add_argument("--out", default=None)
ap.add_argument("--cells", type=int, default=0, help="rehearsal: override the grid size of the part")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
sys.path.insert(1, os.path.join(HERE, "tests"))
import multigrid_jl_amd as mg   # noqa: E402
from complex_cases import complex_rhs, helmholtz, lu_layout   # noqa: E402
from parlu_complex_cases import factor   # noqa: E402
from multigrid_jl_amd.solve_funcs import to_device   # noqa: E402

D = mg.device
lib = D.load_library()
I, F64 = D._i64, D._f64
WARM, REPS, ROUNDS = 3, 10, 5
CYCLES, CYCLE_ROUNDS = 10, 5


def stats(v):
    v = np.asarray(v, dtype=float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def free_bytes():
    torch.cuda.synchronize()
    return int(torch.cuda.mem_get_info()[0])


def form(h, t):
    info = np.zeros(7, dtype=np.int64)
    assert lib.mg_lu_form(h, t, I(info)) == 0, lib.mg_last_error()
    return [int(v) for v in info]


def applier_factor(cells):
    A, _ = helmholtz(mg, [cells, cells])
    A = A.tocsc()
    t0 = time.time()
    G = lu_layout(factor(A))
    print("splu", A.shape[0], "rows", round(time.time() - t0, 2), "s", flush=True)
    return A.shape[0], G


def time_applier(h, n, nrhs, t, words):
    """median of REPS samples; b, x: torch.float64 / float32 [n][nrhs * words] (words: floats or doubles per value)"""
    dt = torch.float64 if words[1] == 8 else torch.float32
    g = torch.Generator(device="cpu").manual_seed(7 + nrhs)
    b = torch.randn(n, nrhs * words[0], dtype=dt, generator=g).cuda()
    x = torch.zeros_like(b)
    torch.cuda.synchronize()
    ms = np.zeros(REPS)
    rc = lib.mg_lu_time_dev(h, b.data_ptr(), x.data_ptr(), n, nrhs, t, WARM, REPS, F64(ms))
    assert rc == 0, lib.mg_last_error()
    assert bool(torch.isfinite(x).all())
    return float(np.median(ms)), x.cpu().numpy()


def part_lu():
    n, G = applier_factor(args.cells or 256)
    S = dict(G, Lv=G["Lv"].astype(np.complex64), Uv=G["Uv"].astype(np.complex64))
    out = dict(n=n, nnzL=int(G["Lp"][-1] - 1), nnzU=int(G["Up"][-1] - 1), handles={}, rows=[])
    H = {}
    for kind, create, Gk, val in (("CFP64", lib.mg_lu_create_CFP64_INT64, G, F64), ("CFP32", lib.mg_lu_create_CFP32_INT64, S, D._f32)):
        f0 = free_bytes()
        h = C.c_void_p()
        rc = create(0, n, I(Gk["Lp"]), I(Gk["Lc"]), val(Gk["Lv"]), I(Gk["Up"]), I(Gk["Uc"]), val(Gk["Uv"]), I(Gk["p"]), I(Gk["q"]), C.byref(h))
        assert rc == 0, lib.mg_last_error()
        f1 = free_bytes()
        fa = form(h, 1)
        f2 = free_bytes()
        H[kind] = h
        out["handles"][kind] = dict(form_plain=form(h, 0), form_adjoint=fa, hbm_plain_set=f0 - f1, hbm_adjoint_set=f1 - f2)
        print("handle", kind, json.dumps(out["handles"][kind]), flush=True)
    words = {"CFP64": (2, 8), "CFP32": (2, 4)}
    samples = {}
    for r in range(ROUNDS):
        for kind in (("CFP64", "CFP32") if r % 2 == 0 else ("CFP32", "CFP64")):     # alternate which handle goes first
            for nrhs in (1, 4, 16):
                for t in (0, 1):
                    med, _ = time_applier(H[kind], n, nrhs, t, words[kind])
                    samples.setdefault((kind, nrhs, t), []).append(med)
    for nrhs in (1, 4, 16):
        for t in (0, 1):
            d, s = stats(samples["CFP64", nrhs, t]), stats(samples["CFP32", nrhs, t])
            row = dict(nrhs=nrhs, doTranspose=t, CFP64_ms=d, CFP32_ms=s, ratio_of_medians=d["median"] / s["median"])
            print("lu", json.dumps(row), flush=True)
            out["rows"].append(row)
    for h in H.values():
        lib.mg_lu_destroy(h)
    return out


def time_cycles(dev, b, x, block=False):
    run = dev.block_cycle_dev if block else dev.cycle_dev
    torch.cuda.synchronize()
    for _ in range(3):
        run(b, x, 1)
    torch.cuda.synchronize()
    ms = []
    for _ in range(CYCLE_ROUNDS):
        t0 = time.perf_counter()
        for _ in range(CYCLES):
            run(b, x, 1)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / CYCLES)
    return ms


def part_cycle():
    PJ = mg.ParallelJuliaSolver
    cells = args.cells or 512
    A, mesh = helmholtz(mg, [cells, cells], 0.5, 0.5)
    n = A.shape[0]
    objects = {"CF64_object": lambda: PJ.getParallelJuliaSolver(np.complex128, np.int64, numCores=2, backend=3),
               "CF32_object": lambda: PJ.getParallelJuliaSolver(np.complex64, np.int64, numCores=2, backend=3, singleFactors=True)}
    P, out = {}, {}
    for name, LU in objects.items():
        p = mg.getMGparam(np.complex128, np.int64, 2, 8, 10, 1e-8, "Jac", 0.8, 2, 2, "V", "NoMUMPS", 0.5, 0.0, singlePrecision=True)
        p.LU = LU()
        t0 = time.perf_counter()
        mg.MGsetup(A, mesh, p)
        out[name] = dict(host_setup_s=time.perf_counter() - t0, rows=[int(M.shape[0]) for M in p.As], cycle_ms_rounds=[])
        f0 = free_bytes()
        dev = to_device(p)
        out[name]["hbm_hierarchy"] = f0 - free_bytes()
        out[name]["coarse_form"] = dev.coarse_form()
        P[name] = p
    b = torch.from_numpy(complex_rhs(n, 9)).cuda()
    for r in range(ROUNDS):
        for name in (tuple(P) if r % 2 == 0 else tuple(P)[::-1]):
            x = torch.zeros_like(b)
            out[name]["cycle_ms_rounds"].append(float(np.median(time_cycles(P[name].device, b, x))))
    bw = complex_rhs(n, 9)
    for name, p in P.items():
        out[name]["cycle_ms"] = stats(out[name]["cycle_ms_rounds"])
        x = np.zeros_like(bw)
        t0 = time.perf_counter()
        _, _, _, resvec = mg.solveGMRES_MG_CFP64(A, p, bw, x, True, 20)
        out[name].update(fgmres_steps=len(resvec), fgmres_s=time.perf_counter() - t0, fgmres_flag=int(p.flag),
                         true_relres=float(np.linalg.norm(bw - A @ x) / np.linalg.norm(bw)))
        print("cycle", name, json.dumps(out[name]), flush=True)
    out["ratio_of_medians"] = out["CF64_object"]["cycle_ms"]["median"] / out["CF32_object"]["cycle_ms"]["median"]
    for p in P.values():
        mg.clear_(p)
    return out


def part_parent():
    out = dict(tree=os.path.abspath(args.root))
    n, G = applier_factor(args.cells or 256)
    h = C.c_void_p()
    rc = lib.mg_lu_create_CFP64_INT64(0, n, I(G["Lp"]), I(G["Lc"]), F64(G["Lv"]), I(G["Up"]), I(G["Uc"]), F64(G["Uv"]), I(G["p"]), I(G["q"]), C.byref(h))
    assert rc == 0, lib.mg_last_error()
    for nrhs in (1, 16):
        for t in (0, 1):
            med, x = time_applier(h, n, nrhs, t, (2, 8))
            out[f"applier_nrhs{nrhs}_t{t}"] = dict(ms=med, sha=sha(x))
    lib.mg_lu_destroy(h)
    c3 = args.cells or 64
    A, mesh = helmholtz(mg, [c3] * 3, 0.25, 0.5)
    p = mg.getMGparam(np.complex128, np.int64, 3, 8, 10, 1e-8, "Jac", 0.8, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(A, mesh, p)
    dev = to_device(p)
    nf = A.shape[0]
    b = torch.from_numpy(complex_rhs(nf, 9)).cuda()
    x = torch.zeros_like(b)
    out["cycle"] = dict(ms=float(np.median(time_cycles(dev, b, x))), sha=sha(x.cpu().numpy()))
    B = torch.from_numpy(np.stack([complex_rhs(nf, 20 + c) for c in range(4)], axis=1).copy()).cuda()
    X = torch.zeros_like(B)
    out["block_cycle_4"] = dict(ms=float(np.median(time_cycles(dev, B, X, block=True))), sha=sha(X.cpu().numpy()))
    mg.clear_(p)
    print("parent", json.dumps(out), flush=True)
    return out


res = {"lu": part_lu, "cycle": part_cycle, "parent": part_parent}[args.part]()
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)
