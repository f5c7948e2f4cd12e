"""Same bits, same speed: the Krylov drivers of two builds of libmgvcycle.so (MGVCYCLE_LIB picks the build of this process) on fixed
seeded problems.  One child process per run; profiles/krylov_host_algebra.md holds the outcome.
    MGVCYCLE_LIB=<lib> python profiles/krylov_host_algebra_measure.py run <driver> <out.npz>     flag, iters, nres, resvec, x of one driver
    MGVCYCLE_LIB=<lib> python profiles/krylov_host_algebra_measure.py speed <out.json>           one warm-up and one timed run per driver
    python profiles/krylov_host_algebra_measure.py compare <dir_a> <dir_b>                       *.npz byte for byte, speed_*.json summarised
Drivers: pcg, bicgstab, fgmres, fgmres_nochain (MG_NO_MGS_CHAIN=1), block_fgmres (2 right-hand sides), vcycle_jacgmres, kcycle on
poisson_shifted([24] * 3); bicgstab_cx, fgmres_cx on case C1 of tests/complex_krylov_oracle.py.
Speed: tol = 0, so FGMRES(10) takes one restart cycle of 10 inner steps and BiCGSTAB 10 iterations; the real drivers on
poisson_shifted([128] * 3) (5 levels, Jac V(1,1)), the complex ones as profiles/complex_krylov_measure.py sets them up."""
import glob
import json
import os
import sys
import time

import torch
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

REAL = ("pcg", "bicgstab", "fgmres", "fgmres_nochain", "block_fgmres", "vcycle_jacgmres", "kcycle")
COMPLEX = ("bicgstab_cx", "fgmres_cx")


def run(driver, out_path):
    if driver == "fgmres_nochain":
        os.environ["MG_NO_MGS_CHAIN"] = "1"                     # read when the handle is created
    import multigrid_jl_amd as mg
    if driver in COMPLEX:
        import complex_krylov_oracle as ck
        p, As, b = ck.case(mg, "C1")
        dev = mg.to_device(p)
        dev.set_krylov_operator(As)
        x = np.zeros_like(b)
        if driver == "bicgstab_cx":
            _, flag, it, rv = dev.bicgstab(b, x, ck.TOL, ck.MAXIT_BICGSTAB)
        else:
            _, flag, it, rv = dev.fgmres(b, x, 5, ck.TOL, ck.MAXIT_FGMRES)
    else:
        A, mesh = mg.poisson_shifted([24, 24, 24])
        nrhs = 2 if driver == "block_fgmres" else 1
        relax, cyc = {"vcycle_jacgmres": ("Jac-GMRES", "V"), "kcycle": ("Jac", "K")}.get(driver, ("Jac", "V"))
        p = mg.getMGparam(np.float64, np.int64, 3, 8, 12, 1e-9, relax, 0.8, 1, 1, cyc, "NoMUMPS", 0.5, 0.0)
        mg.MGsetup(A, mesh, p, nrhs)
        b = np.asfortranarray(mg.seeded_rhs(A, nrhs)) if nrhs > 1 else mg.seeded_rhs(A)
        x = np.zeros_like(b, order="F")
        if driver == "pcg":
            _, _, it = mg.solveCG_MG(A, p, b, x)
        elif driver == "bicgstab":
            _, _, it, _ = mg.solveBiCGSTAB_MG(A, p, b, x)
        elif driver in ("fgmres", "fgmres_nochain", "block_fgmres"):
            _, _, it, _ = mg.solveGMRES_MG(A, p, b, x, True, 5)
        else:
            _, _, it = mg.solveMG(p, b, x)
        flag, rv = getattr(p, "flag", 0), np.asarray(p.resvec)
    rv = np.asarray(rv)
    np.savez(out_path, flag=np.int64(flag), iters=np.int64(it), nres=np.int64(rv.shape[0]), resvec=rv, x=np.asarray(x))
    print(driver, "flag", flag, "iters", it, "nres", rv.shape[0], "last", rv.reshape(rv.shape[0], -1)[-1].max(), flush=True)


def speed(out_path):
    import multigrid_jl_amd as mg
    import complex_krylov_measure as ckm
    out = {}
    A, mesh = mg.poisson_shifted([128] * 3)
    p = mg.getMGparam(np.float64, np.int64, 5, 8, ckm.ITERS, 0.0, "Jac", 0.8, 1, 1, "V", "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(A, mesh, p)
    b = mg.seeded_rhs(A)
    for method in ("fgmres", "bicgstab"):
        for timed in (False, True):                              # one warm-up, one timed run
            x = np.zeros_like(b)
            p.maxOuterIter = 1 if method == "fgmres" else ckm.ITERS
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            it = mg.solveGMRES_MG(A, p, b, x, True, ckm.INNER)[2] if method == "fgmres" else mg.solveBiCGSTAB_MG(A, p, b, x)[2]
            torch.cuda.synchronize()
            if timed:
                out[method] = dict(iterations=int(it), ms_per_iter=1e3 * (time.perf_counter() - t0) / it)
    mg.clear_(p)
    pc, dev, As, bc, _ = ckm.setup()
    bt = torch.from_numpy(bc).cuda()
    xt = torch.zeros(bc.shape[0], dtype=torch.complex128, device="cuda")
    for method in ("fgmres", "bicgstab"):
        for timed in (False, True):
            s, it = ckm.device_run(dev, method, bt, xt)
            if timed:
                out[method + "_cx"] = dict(iterations=int(it), ms_per_iter=1e3 * s / it)
    mg.clear_(pc)
    print(json.dumps(out), flush=True)
    json.dump(out, open(out_path, "w"), indent=1)


def compare(dir_a, dir_b):
    """Every array of every <driver>.npz byte for byte; the speed files as median (min - max) over the repetitions of each build."""
    same = True
    for d in REAL + COMPLEX:
        if not os.path.exists(os.path.join(dir_a, d + ".npz")):    # (a directory of speed files only)
            continue
        a, b = np.load(os.path.join(dir_a, d + ".npz")), np.load(os.path.join(dir_b, d + ".npz"))
        diff = [k for k in a.files if a[k].tobytes() != b[k].tobytes()]
        same = same and not diff
        print(f"{d:16s} flag {int(a['flag']):3d} iters {int(a['iters']):3d} nres {int(a['nres']):3d}  "
              + ("identical" if not diff else "DIFFERENT: " + ", ".join(f"{k} max|diff| {np.abs(a[k] - b[k]).max():.3e}" for k in diff)))
    for name, d in (("a", dir_a), ("b", dir_b)):
        recs = [json.load(open(f)) for f in sorted(glob.glob(os.path.join(d, "speed_*.json")))]
        for key in (recs[0] if recs else {}):
            v = [r[key]["ms_per_iter"] for r in recs]
            print(f"{name} {key:12s} {len(v)} runs of {recs[0][key]['iterations']:2d}: median {np.median(v):.3f} ms per iteration (min {min(v):.3f}, max {max(v):.3f})")
    return 0 if same else 1


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "run":
        run(sys.argv[2], sys.argv[3])
    elif mode == "speed":
        speed(sys.argv[2])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
