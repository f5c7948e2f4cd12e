"""Measurements behind profiles/coarse_solver.md (the coarsest solve by a solver object).
    python profiles/coarse_solver_measure.py PART [--root TREE] [--out FILE.json]
PART:
  sweep0  one Schwarz sweep from x = 0 on the problem of profiles/dd_schwarz_measure.py (64 x 64 x 32 cells, boxes [8,8,4],
          overlap 1: eight batched colours), FP64 and CFP64: the from-zero form against a zero fill + the ordinary sweep
          (mg_dd0_time_dev: events on the handle's stream), alternating, ROUNDS rounds of REPS samples each.  The form was
          not faster and is not in the library: apply profiles/coarse_solver_from_zero_variant.patch and rebuild first;
  lu      ms per mg_cycle_dev_CFP64 of a 2-level 2-D Helmholtz hierarchy on 512^2 cells, whose coarsest level (257^2 = 66 049
          rows) is held as sparse factors.  Uses only what the parent commit has too: --root names the tree whose package
          (and built library) is imported, so one job times the parent and this commit;
  dd      the same hierarchy with a Schwarz sweep as coarsest solve (boxes [8,8], overlap [1,1]): ms per cycle, launches per
          coarse solve, and the BiCGSTAB iteration count to 1e-6 against the exact-LU hierarchy.
Cycle times: host clock around CYCLES enqueued cycles ending in a device synchronise, after a warm-up."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch
import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("part", choices=["sweep0", "lu", "dd"])
ap.add_argument("--root", default=HERE)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
sys.path.insert(1, os.path.join(HERE, "tests"))
import multigrid_jl_amd as mg   # noqa: E402
import dd_cases                  # noqa: E402
from complex_cases import complex_rhs, helmholtz   # noqa: E402

D = mg.device
REPS, WARM, ROUNDS = 30, 5, 5
CYCLES, CYCLE_ROUNDS = 10, 7


def stats(v):
    v = np.asarray(v, dtype=float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def part_sweep0():
    if "mg_dd0_time_dev" not in D.SIGNATURES:
        sys.exit("sweep0 measures a variant that is not in the library: apply profiles/coarse_solver_from_zero_variant.patch and rebuild")
    lib = D.load_library()
    out = {}
    for cx in (False, True):
        n, boxes, ov = [64, 64, 32], [8, 8, 4], [1, 1, 1]
        A, mesh, b = dd_cases.poisson(mg, n, seed=1)
        if cx:
            A = (A.astype(np.complex128) - (1.0 - 0.5j) * 0.25 * (A.diagonal().max() / 6) * sp.identity(A.shape[0])).tocsr()
            A.sort_indices()
            b = b + 1j * np.random.default_rng(9).standard_normal(A.shape[0])
        p = dd_cases.dd_param(mg, A, mesh, boxes, ov, VAL=np.complex128 if cx else np.float64)
        info = mg.DomainDecomposition.ddInfo(p, A)
        h = p._handle
        bd = torch.from_numpy(b).cuda()
        xd = torch.zeros_like(bd)
        torch.cuda.synchronize()
        ms = (C.c_double * REPS)()
        rounds = {0: [], 1: []}
        for r in range(ROUNDS):
            for from_zero in ((0, 1) if r % 2 == 0 else (1, 0)):      # alternate which form goes first
                D._check(lib, lib.mg_dd0_time_dev(h, D._ptr(bd), D._ptr(xd), A.shape[0], 0, from_zero, WARM, REPS, ms), "mg_dd0_time_dev")
                rounds[from_zero].append(float(np.median(list(ms))))
        rec = dict(rows=int(A.shape[0]), info=info, zero_fill_plus_sweep_ms=rounds[0], from_zero_ms=rounds[1],
                   zero_fill_plus_sweep=stats(rounds[0]), from_zero=stats(rounds[1]))
        rec["gain_of_medians"] = 1.0 - rec["from_zero"]["median"] / rec["zero_fill_plus_sweep"]["median"]
        out["CFP64" if cx else "FP64"] = rec
        print("sweep0", "CFP64" if cx else "FP64", json.dumps(rec), flush=True)
        p.close()
    return out


def hierarchy(LU=None):
    A, mesh = helmholtz(mg, [512, 512], 0.5, 0.5)
    p = mg.getMGparam(np.complex128, np.int64, 2, 8, 200, 1e-6, "Jac", 0.8, 2, 2, "V", "NoMUMPS", 0.5, 0.0)
    p.LU = LU(mesh) if LU else None
    t0 = time.perf_counter()
    mg.MGsetup(A, mesh, p)
    return A, p, time.perf_counter() - t0


def time_cycles(dev, n):
    b = torch.from_numpy(complex_rhs(n, 9)).cuda()
    x = torch.zeros_like(b)
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
    return stats(ms), x.cpu().numpy()


def part_lu():
    A, p, setup_s = hierarchy()
    dev = D.DeviceHierarchy(p)
    rec = dict(tree=os.path.abspath(args.root), rows=[int(M.shape[0]) for M in p.As], host_setup_s=setup_s)
    if hasattr(dev, "coarse_form"):
        rec["coarse_form"] = dev.coarse_form()
    rec["cycle_ms"], x = time_cycles(dev, A.shape[0])
    rec["x_norm"] = float(np.linalg.norm(x))          # the same number from both trees: the cycles compute the same thing
    dev.close()
    print("lu", json.dumps(rec), flush=True)
    return rec


def part_dd():
    import coarse_solver_cases as cs
    out = {}
    for name, LU in (("exact_lu", None), ("schwarz", lambda mesh: cs.dd_lu(mg, mesh, [8, 8], [1, 1], np.complex128))):
        A, p, setup_s = hierarchy(LU)
        b = complex_rhs(A.shape[0], 9)
        x = np.zeros_like(b)
        t0 = time.perf_counter()
        _, _, it, _ = mg.solveBiCGSTAB_MG_CFP64(A, p, b, x)
        solve_s = time.perf_counter() - t0
        rec = dict(host_setup_s=setup_s, coarse_form=p.device.coarse_form(), bicgstab_iterations=int(it), bicgstab_flag=int(p.flag),
                   bicgstab_s=solve_s, true_relres=float(np.linalg.norm(b - A @ x) / np.linalg.norm(b)))
        rec["cycle_ms"], _ = time_cycles(p.device, A.shape[0])
        out[name] = rec
        print("dd", name, json.dumps(rec), flush=True)
        mg.clear_(p)
    return out


res = {"sweep0": part_sweep0, "lu": part_lu, "dd": part_dd}[args.part]()
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)
