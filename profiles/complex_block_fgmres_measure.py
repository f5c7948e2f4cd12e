"""Complex block FGMRES against block BiCGSTAB and the single-vector FGMRES, and its Gram kernels against the block BiCGSTAB driver's,
on the problem of profiles/complex_block_measure.py: shifted Laplacian at 128^3 cells (k h = 0.25, damping 0.5, four levels, SPAI,
V(2,1)), system operator with damping 0.05, CF64 hierarchy.
    python profiles/complex_block_fgmres_measure.py steps [out.json]   for k in 2, 4, 8, 16: ms per column of one block FGMRES(10)
                                                   inner step (one restart of 10 steps, tol = 0), of one block BiCGSTAB iteration, and
                                                   of one single-vector FGMRES(10) inner step; one warm-up, then 5 rounds, the three
                                                   alternating inside every round; then steps / iterations to 1e-8
    python profiles/complex_block_fgmres_measure.py kernels            per k: 2 block BiCGSTAB iterations, then one restart of block
                                                   FGMRES(10), 3 rounds - the run to put under rocprofv3 --kernel-trace
    python profiles/complex_block_fgmres_measure.py stats <kernel_trace.csv>   per k (the sections are told apart by the k rows of
                                                   cx_blk_gram_partial's grid, BiCGSTAB first in every section): calls, median, min,
                                                   max of the Gram and combination kernels, the achieved rate against the byte
                                                   models, and the share of block FGMRES's kernel time spent in orthogonalisation
    python profiles/complex_block_fgmres_measure.py parent [out.json]  what the parent commit has: ms and a checksum of the bits of one
                                                   V(2,1) single cycle, one 4-column block cycle and 5 iterations of 4-column block
                                                   BiCGSTAB; run it from both trees, alternating, and compare
CBF_CELLS overrides the 128 (rehearsals), CBF_K the list of column counts."""
import csv
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.environ.get("CBF_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multigrid_jl_amd as mg                    # noqa: E402
from complex_cases import complex_rhs, helmholtz  # noqa: E402

CELLS = int(os.environ.get("CBF_CELLS", "128"))
KS = [int(t) for t in os.environ.get("CBF_K", "2,4,8,16").split(",")]
INNER, ITERS, REPS, WARM = 10, 5, 5, 1
TOL = 1e-8


def build():
    Ah, mesh = helmholtz(mg, [CELLS] * 3, 0.25, 0.5)
    p = mg.getMGparam(np.complex128, np.int64, 4, 8, ITERS, 0.0, "SPAI", 1.0, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(Ah, mesh, p)
    As, _ = helmholtz(mg, [CELLS] * 3, 0.25, 0.05)
    dev = mg.device.DeviceHierarchy(p)
    dev.set_krylov_operator(As)
    return p, As, dev


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def block(n, k):
    B = np.ascontiguousarray(np.stack([complex_rhs(n, 40 + j) for j in range(k)], axis=1))     # row-major [n][k]
    Bt = torch.from_numpy(B).cuda()
    return B, Bt, torch.zeros_like(Bt)


def summary(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def steps(out_path):
    p, As, dev = build()
    n = As.shape[0]
    out = dict(cells=CELLS, n=n, inner=INNER, reps=REPS)
    bt1 = torch.from_numpy(complex_rhs(n, 40)).cuda()
    xt1 = torch.zeros_like(bt1)

    def single_steps(tol=0.0, maxit=1):
        xt1.zero_()
        return dev.fgmres_dev(bt1, xt1, INNER, tol, maxit)

    for k in KS:
        B, Bt, Xt = block(n, k)

        def fgmres_steps(tol=0.0, maxit=1):
            Xt.zero_()
            return dev.block_fgmres_dev_CFP64(Bt, Xt, INNER, tol, maxit)

        def bicgstab_iters(tol=0.0, maxit=ITERS):
            Xt.zero_()
            return dev.block_bicgstab_dev_CFP64(Bt, Xt, tol, maxit)

        t = dict(block_fgmres_step=[], block_bicgstab_iter=[], single_fgmres_step=[])
        for rep in range(WARM + REPS):
            a = timed(fgmres_steps)[0]
            b_ = timed(bicgstab_iters)[0]
            c = timed(single_steps)[0]
            if rep >= WARM:
                t["block_fgmres_step"].append(1e3 * a / (INNER * k))
                t["block_bicgstab_iter"].append(1e3 * b_ / (ITERS * k))
                t["single_fgmres_step"].append(1e3 * c / INNER)
        r = {w: summary(v) for w, v in t.items()}
        s, (flag, count, _rv) = timed(lambda: fgmres_steps(TOL, 40))
        X = Xt.cpu().numpy()
        r["block_fgmres_to_tol"] = dict(steps=count, flag=flag, seconds=s, true_residual=float(np.linalg.norm(B - As @ X) / np.linalg.norm(B)))
        s, (flag, count, _rv) = timed(lambda: bicgstab_iters(TOL, 200))
        X = Xt.cpu().numpy()
        r["block_bicgstab_to_tol"] = dict(iterations=count, flag=flag, seconds=s,
                                          worst_true_residual=float((np.linalg.norm(B - As @ X, axis=0) / np.linalg.norm(B, axis=0)).max()))
        print(k, json.dumps(r), flush=True)
        out[str(k)] = r
        del Bt, Xt
        torch.cuda.empty_cache()
    s, (flag, count, _rv) = timed(lambda: single_steps(TOL, 40))
    out["single_fgmres_to_tol"] = dict(steps=count, flag=flag, seconds=s)
    print("single", json.dumps(out["single_fgmres_to_tol"]), flush=True)
    dev.close()
    if out_path:
        json.dump(out, open(out_path, "w"), indent=1)


def kernels():
    p, As, dev = build()
    n = As.shape[0]
    for k in KS:
        B, Bt, Xt = block(n, k)
        for _ in range(3):
            Xt.zero_()
            dev.block_bicgstab_dev_CFP64(Bt, Xt, 0.0, 2)
            Xt.zero_()
            dev.block_fgmres_dev_CFP64(Bt, Xt, INNER, 0.0, 1)
        torch.cuda.synchronize()
        print("traced k =", k, flush=True)
        del Bt, Xt
        torch.cuda.empty_cache()
    dev.close()


def stats(path):
    n = (CELLS + 1) ** 3
    rows = []
    for r in csv.DictReader(open(path)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"], int(r.get("Grid_Size_Y") or 1)))
    rows.sort()
    k, sect = None, {}
    for start, dur, name, gy in rows:
        if "cx_blk_gram_partial" in name:
            k = gy
        if k is not None:
            sect.setdefault(k, []).append((name, dur))
    for k, items in sorted(sect.items()):
        by = {}
        for name, dur in items:
            for key in ("cx_blk_gram_partial", "cx_blk_gram_final_wave", "cx_blk_gram_final", "cx_blk_gram_onepass", "cx_blk_comb_gram", "cx_blk_comb"):
                if key in name:                                  # (the longer of two names that share a prefix is tried first)
                    by.setdefault(key, []).append(dur / 1e3)
                    break
        print(f"k = {k}")
        for key, v in by.items():
            line = f"  {key:22s} calls {len(v):4d}  median {np.median(v):9.1f} us  min {min(v):9.1f}  max {max(v):9.1f}"
            if key in ("cx_blk_gram_partial", "cx_blk_gram_onepass"):
                line += f"  | model 2nk16 = {2 * n * k * 16 / 1e6:.1f} MB -> {2 * n * k * 16 / (np.median(v) * 1e-6) / 1e12:.2f} TB/s at the median"
            print(line)
        # the orthogonalisation's share of block FGMRES: the section's last restart runs from the first one-pass Gram behind the
        # last cx_blk_gram_partial (block BiCGSTAB's) to the section's end
        last = max(i for i, (nm, _) in enumerate(items) if "cx_blk_gram_partial" in nm)
        seg = items[last + 1:]
        first = next((i for i, (nm, _) in enumerate(seg) if "cx_blk_gram_onepass" in nm), None)
        if first is not None:
            seg = seg[first:]
            tot = sum(d for _, d in seg)
            orth = sum(d for nm, d in seg if "cx_blk_" in nm)
            print(f"  kernel time of the last block FGMRES(10) restart: {tot / 1e6:.2f} ms, of it the cx_blk_* kernels (Gram matrices, "
                  f"updates, Cholesky QR, X update) {orth / 1e6:.2f} ms ({100 * orth / tot:.1f} %)")


def parent(out_path):
    p, As, dev = build()
    n = As.shape[0]
    digest = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16]
    bt1 = torch.from_numpy(complex_rhs(n, 40)).cuda()
    xt1 = torch.zeros_like(bt1)
    B, Bt, Xt = block(n, 4)
    jobs = dict(single_cycle=lambda: [dev.cycle_dev(bt1, xt1, 1) for _ in range(10)],
                block_cycle_4=lambda: [dev.block_cycle_dev(Bt, Xt, 1) for _ in range(10)],
                block_bicgstab_4=lambda: (Xt.zero_(), dev.block_bicgstab_dev_CFP64(Bt, Xt, 0.0, ITERS)))
    div = dict(single_cycle=10, block_cycle_4=10, block_bicgstab_4=ITERS)
    t = {w: [] for w in jobs}
    for rep in range(WARM + REPS):
        for w, fn in jobs.items():
            s = timed(fn)[0]
            if rep >= WARM:
                t[w].append(1e3 * s / div[w])
    out = {w: summary(v) for w, v in t.items()}
    jobs["single_cycle"]()
    torch.cuda.synchronize()
    out["bits"] = dict(single_cycle=digest(xt1))
    jobs["block_cycle_4"]()
    torch.cuda.synchronize()
    out["bits"]["block_cycle_4"] = digest(Xt)
    res = jobs["block_bicgstab_4"]()[1]
    torch.cuda.synchronize()
    out["bits"]["block_bicgstab_4"] = digest(Xt)
    out["bits"]["block_bicgstab_4_resvec"] = hashlib.sha256(np.asarray(res[2]).tobytes()).hexdigest()[:16]
    print(ROOT, json.dumps(out), flush=True)
    dev.close()
    if out_path:
        json.dump(out, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "steps"
    arg = sys.argv[2] if len(sys.argv) > 2 else None
    {"steps": steps, "kernels": lambda _: kernels(), "stats": stats, "parent": parent}[mode](arg)
