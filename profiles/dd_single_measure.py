"""The Float32 / ComplexF32 Schwarz sweep against the Float64 / ComplexF64 one (mg_dd_time_dev: events on the handle's stream).
    python profiles/dd_single_measure.py PART [--root TREE] [--out FILE.json] [--cells N]
  sweep2d  one sweep on 512 x 512 cells in 16 x 16 boxes, overlap 1 (one launch per colour): Poisson FP64 / FP32 and damped
           Helmholtz CFP64 / CFP32 - ms per sweep and the HBM each handle keeps resident;
  sweep3d  the same on 64^3 cells in 4 x 4 x 4 boxes (members of 18^3 rows: each an applier of its own, the sequential path);
  cycle    the 2-level ComplexF32 hierarchy of profiles/parlu_single.md on 512 x 512 cells with a ComplexF32 sweep as coarsest
           solve against the ComplexF64 hierarchy with the ComplexF64 sweep: ms per cycle and FGMRES(20) steps to 1e-8;
  parent   run with --root on a checkout of the parent commit and on this tree in the same job: the FP64 and CFP64 sweeps of
           sweep2d and of 32^3 cells in 4 x 4 x 4 boxes - ms and a SHA-256 of the iterate after one sweep from zero.
Times: medians of ROUNDS alternating rounds (each the median of REPS samples) with min and max.  Resident bytes: the drop of free
device memory over the handle's creation (operator, index lists, factors of the plain direction, work vectors)."""
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
ap.add_argument("part", choices=["sweep2d", "sweep3d", "cycle", "parent"])
ap.add_argument("--root", default=HERE)
ap.add_argument("--out", default=None)
ap.add_argument("--cells", type=int, default=0, help="rehearsal: override the grid size of the part")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
sys.path.insert(1, os.path.join(HERE, "tests"))
import multigrid_jl_amd as mg   # noqa: E402
import dd_cases                  # noqa: E402
from complex_cases import complex_rhs, helmholtz   # noqa: E402
from multigrid_jl_amd.solve_funcs import to_device   # noqa: E402

D = mg.device
DD = mg.DomainDecomposition
PJ = mg.ParallelJuliaSolver
lib = D.load_library()
WARM, REPS, ROUNDS = 3, 10, 5
CYCLES, CYCLE_ROUNDS = 10, 5
WIDE = {np.float32: np.float64, np.complex64: np.complex128}


def stats(v):
    v = np.asarray(v, dtype=float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def free_bytes():
    torch.cuda.synchronize()
    return int(torch.cuda.mem_get_info()[0])


def shape(part):
    if part == "sweep2d":
        c = args.cells or 512
        return [c, c], [c // 32, c // 32], [1, 1]
    c = args.cells or 64
    return [c, c, c], [4, 4, 4], [1, 1, 1]


def problem(cells, cx):
    """(A, mesh, b) in double: the Poisson problem of dd_cases, or the damped Helmholtz operator of complex_cases."""
    if cx:
        A, mesh = helmholtz(mg, cells, 0.5, 0.5)
        return A, mesh, complex_rhs(A.shape[0], 9)
    return dd_cases.poisson(mg, cells, seed=1)


def dd_param(A, mesh, boxes, ov, VAL):
    """A set-up DDparam of VAL on A (A already of VAL)."""
    if VAL in WIDE:
        Ainv = PJ.getParallelJuliaSolver(VAL, np.uint32 if VAL is np.float32 else np.int64, singleFactors=True)
        p = mg.getDomainDecompositionParam(VAL, np.int64, mesh, boxes, ov, mg.getNodalIndicesOfCell, Ainv, singleValues=True)
        return mg.setupDDSerial(A, p)
    return dd_cases.dd_param(mg, A, mesh, boxes, ov, VAL=VAL)


def handle(A, mesh, b, boxes, ov, VAL):
    Av = A.astype(VAL).tocsr()
    t0 = time.perf_counter()
    p = dd_param(Av, mesh, boxes, ov, VAL)
    setup_s = time.perf_counter() - t0
    f0 = free_bytes()
    info = DD.ddInfo(p, Av)                      # creates and finalizes the device handle
    resident = f0 - free_bytes()
    info = {k: (v if not isinstance(v, type) else np.dtype(v).name) for k, v in info.items()}
    bd = torch.from_numpy(np.ascontiguousarray(b, dtype=VAL)).cuda()
    return dict(p=p, A=Av, b=bd, x=torch.zeros_like(bd), info=info, resident_bytes=resident, host_setup_s=setup_s,
                max_sub_rows=int(max(len(g) for g in p.GlobalIndices)))


def time_sweep(H):
    H["x"].zero_()
    torch.cuda.synchronize()
    ms = (C.c_double * REPS)()
    D._check(lib, lib.mg_dd_time_dev(H["p"]._handle, D._ptr(H["b"]), D._ptr(H["x"]), H["A"].shape[0], 0, WARM, REPS, ms), "mg_dd_time_dev")
    assert bool(torch.isfinite(torch.view_as_real(H["x"]) if H["x"].is_complex() else H["x"]).all())
    return float(np.median(list(ms)))


def first_sweep(H):
    H["x"].zero_()
    torch.cuda.synchronize()
    mg.solveDDSerial(H["A"], H["b"], H["x"], H["p"], 1, 0)
    torch.cuda.synchronize()
    return H["x"].cpu().numpy()


def part_sweep(part):
    cells, boxes, ov = shape(part)
    out = dict(cells=cells, boxes=boxes, overlap=ov, pairs={})
    for cx, (wide, single) in ((False, (np.float64, np.float32)), (True, (np.complex128, np.complex64))):
        A, mesh, b = problem(cells, cx)
        H = {np.dtype(V).name: handle(A, mesh, b, boxes, ov, V) for V in (wide, single)}
        names = tuple(H)
        rounds = {k: [] for k in names}
        for r in range(ROUNDS):
            for k in (names if r % 2 == 0 else names[::-1]):            # alternate which handle goes first
                rounds[k].append(time_sweep(H[k]))
        xw, xs = first_sweep(H[names[0]]), first_sweep(H[names[1]])
        rec = {k: dict(ms=stats(rounds[k]), resident_bytes=H[k]["resident_bytes"], info=H[k]["info"], host_setup_s=H[k]["host_setup_s"],
                       max_sub_rows=H[k]["max_sub_rows"]) for k in names}
        rec.update(rows=int(A.shape[0]), time_ratio_double_over_single=rec[names[0]]["ms"]["median"] / rec[names[1]]["ms"]["median"],
                   bytes_ratio_single_over_double=rec[names[1]]["resident_bytes"] / rec[names[0]]["resident_bytes"],
                   first_sweep_rel_diff=float(np.abs(xs - xw).max() / np.abs(xw).max()))
        print(part, "complex" if cx else "real", json.dumps(rec), flush=True)
        out["pairs"]["complex" if cx else "real"] = rec
        for h in H.values():
            h["p"].close()
    return out


def time_cycles(dev, b, x):
    torch.cuda.synchronize()
    for _ in range(3):
        dev.cycle_dev(b, x, 1)
    torch.cuda.synchronize()
    ms = []
    for _ in range(CYCLE_ROUNDS):
        t0 = time.perf_counter()
        for _ in range(CYCLES):
            dev.cycle_dev(b, x, 1)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / CYCLES)
    return ms


def part_cycle():
    cells = args.cells or 512
    A, mesh = helmholtz(mg, [cells, cells], 0.5, 0.5)
    n = A.shape[0]
    boxes, ov = [cells // 32, cells // 32], [1, 1]                      # on the coarsest grid of cells/2: boxes of 16 cells
    dd32 = lambda: mg.getDomainDecompositionParam(np.complex64, np.int64, mesh, boxes, ov, mg.getNodalIndicesOfCell,
                                                  PJ.getParallelJuliaSolver(np.complex64, np.int64, singleFactors=True), singleValues=True)
    dd64 = lambda: mg.getDomainDecompositionParam(np.complex128, np.int64, mesh, boxes, ov, mg.getNodalIndicesOfCell,
                                                  PJ.getParallelJuliaSolver(np.complex128, np.int64))
    P, out = {}, {}
    for name, LU, single in (("CF64_pair", dd64, False), ("CF32_pair", dd32, True)):
        p = mg.getMGparam(np.complex128, np.int64, 2, 8, 10, 1e-8, "Jac", 0.8, 2, 2, "V", "NoMUMPS", 0.5, 0.0, singlePrecision=single)
        p.LU = LU()
        t0 = time.perf_counter()
        mg.MGsetup(A, mesh, p)
        out[name] = dict(host_setup_s=time.perf_counter() - t0, rows=[int(M.shape[0]) for M in p.As], cycle_ms_rounds=[])
        f0 = free_bytes()
        dev = to_device(p)
        out[name]["hbm_hierarchy_and_sweep"] = f0 - free_bytes()
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
    out["ratio_of_medians"] = out["CF64_pair"]["cycle_ms"]["median"] / out["CF32_pair"]["cycle_ms"]["median"]
    for p in P.values():
        mg.clear_(p)
    return out


def part_parent():
    """The double sweeps of a tree (this one or the parent commit's): times and the bits of the first sweep."""
    out = dict(tree=os.path.abspath(args.root))
    c2, c3 = args.cells or 512, (args.cells or 64) // 2                 # (3-D at half the size: the host factorises every tree's boxes)
    for part, (cells, boxes, ov) in (("sweep2d", ([c2, c2], [c2 // 32, c2 // 32], [1, 1])), ("sweep3d_half", ([c3] * 3, [4, 4, 4], [1, 1, 1]))):
        for cx, VAL in ((False, np.float64), (True, np.complex128)):
            A, mesh, b = problem(cells, cx)
            H = handle(A, mesh, b, boxes, ov, VAL)
            ms = [time_sweep(H) for _ in range(ROUNDS)]
            out[f"{part}_{np.dtype(VAL).name}"] = dict(ms=stats(ms), sha=sha(first_sweep(H)), resident_bytes=H["resident_bytes"])
            H["p"].close()
    print("parent", json.dumps(out), flush=True)
    return out


res = {"sweep2d": lambda: part_sweep("sweep2d"), "sweep3d": lambda: part_sweep("sweep3d"), "cycle": part_cycle,
       "parent": part_parent}[args.part]()
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)
