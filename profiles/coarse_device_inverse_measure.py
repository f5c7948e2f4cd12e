"""Measurements behind profiles/coarse_device_inverse.md (the coarsest operator's explicit inverse built on the device).
    python profiles/coarse_device_inverse_measure.py standalone [--sizes 125,729,4913,8192] [--out FILE.json]
    python profiles/coarse_device_inverse_measure.py hier [--out FILE.json]
    python profiles/coarse_device_inverse_measure.py vanka [--out FILE.json]
    python profiles/coarse_device_inverse_measure.py unchanged [--root TREE] [--out FILE.json]
standalone  device.dense_inverse (host matrix in, host inverse out: the copies are inside the time) against the host route of
            _set_coarse - splu(A).solve(eye) - and numpy.linalg.inv on the same matrix, ComplexF64 and Float64: shifted nodal
            Laplacians of 5^3, 9^3, 17^3 and 16*16*32 points (125, 729, 4913, 8192 rows).  ROUNDS alternating rounds (device, host,
            numpy, device, ...); at 8192 rows the two host routes run once.  torch.linalg.inv on the device where it runs.
hier        128^3 cells, four levels, SPAI, ComplexF64 (coarsest 4913 rows; the hierarchy of profiles/complex_rap.md): per round and
            per param (flag off / flag on, alternating) replaceMatrixInHierarchy plus the first following cycle, the upload plus the
            first cycle, the median of 20 cycles; the parts of replace_matrix (timings).  CDI_CELLS overrides the 128 (rehearsals).
vanka       64^3 cells, four levels, Vanka hierarchy with vankaDeviceSetup (profiles/vanka_device_setup.md), with and without
            coarseDeviceInverse: replaceMatrixInHierarchy plus the first cycle.  CDI_VANKA_CELLS overrides the 64.
unchanged   one tree (--root names the tree whose package and built library are imported, so the parent commit is timed by the same
            script): the V(2,1) Jac dense-inverse ComplexF64 cycle at 64^3 cells, its 4-column block cycle and a Float64 V(2,1) Jac
            cycle - sha256 of the result and the median of 30 calls each."""
import argparse
import hashlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("part", choices=["standalone", "hier", "vanka", "unchanged"])
ap.add_argument("--root", default=HERE)
ap.add_argument("--sizes", default="125,729,4913,8192")
ap.add_argument("--out", default=None)
args = ap.parse_args()
ROUNDS = 5
sys.path.insert(0, os.path.abspath(args.root))
sys.path.insert(1, os.path.join(HERE, "tests"))
import torch  # noqa: E402,F401  (first: it bundles its own HIP runtime)
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import scipy.sparse.linalg as spla  # noqa: E402
import multigrid_jl_amd as mg  # noqa: E402

GRIDS = {125: [4, 4, 4], 729: [8, 8, 8], 4913: [16, 16, 16], 8192: [15, 15, 31]}


def stats(v):
    v = np.asarray(v, dtype=float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(v.size))


def shifted(cells, cx):
    mesh = mg.getRegularMesh([0.0, 1.0] * 3, list(cells))
    L = mg.getNodalLaplacianMatrix(mesh).tocsr()
    k2 = 0.25 * L.diagonal().max() / 6.0
    shift = (1.0 - 0.5j) * k2 if cx else -k2
    A = (L.astype(np.complex128 if cx else np.float64) - shift * sp.identity(L.shape[0], format="csr")).tocsr()
    A.sort_indices()
    return A, mesh


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


def res(A, X):
    n = A.shape[0]
    return max(np.linalg.norm(A @ X - np.eye(n)), np.linalg.norm(X @ A - np.eye(n))) / np.sqrt(n)


def part_standalone():
    out = []
    mg.device.dense_inverse(np.eye(4))                      # (library load, context)
    for n in [int(s) for s in args.sizes.split(",")]:
        for cx in (True, False):
            As, _ = shifted(GRIDS[n], cx)
            assert As.shape[0] == n
            Ad = np.asfortranarray(As.toarray())
            host_rounds = ROUNDS if n <= 4913 else 1
            dev, host, npy, tor = [], [], [], []
            X = mg.device.dense_inverse(Ad)                 # unrecorded first call
            for r in range(ROUNDS):
                dev.append(timed(lambda: mg.device.dense_inverse(Ad))[0])
                if r < host_rounds:
                    host.append(timed(lambda: spla.splu(sp.csc_matrix(As)).solve(np.eye(n, dtype=Ad.dtype)))[0])
                    t, Xn = timed(lambda: np.linalg.inv(Ad))
                    npy.append(t)
            try:
                T = torch.as_tensor(np.ascontiguousarray(Ad)).cuda()
                torch.linalg.inv(T)
                torch.cuda.synchronize()
                for r in range(ROUNDS):
                    t0 = time.perf_counter()
                    torch.linalg.inv(T)
                    torch.cuda.synchronize()
                    tor.append(time.perf_counter() - t0)
            except Exception as e:                          # a yardstick only: not a dependency
                tor = None
                print("torch.linalg.inv did not run:", repr(e)[:200])
            flops = (8.0 if cx else 2.0) * n ** 3
            rec = dict(n=n, complex=cx, device_s=stats(dev), host_lu_solve_eye_s=stats(host), numpy_inv_s=stats(npy),
                       torch_inv_device_s=stats(tor) if tor else None, flops=flops, device_flops_per_s=flops / np.median(dev),
                       res_device=res(Ad, X), res_numpy=res(Ad, Xn), cond=float(np.linalg.cond(Ad)) if n <= 729 else None)
            print(json.dumps(rec), flush=True)
            out.append(rec)
    return out


def _copy_param(p, **fields):
    import copy
    q = copy.copy(p)
    q.As, q.Ps, q.Rs = [M.copy() for M in p.As], list(p.Ps), list(p.Rs)
    q.relaxPrecs = [np.array(d) for d in p.relaxPrecs]
    q.device = None
    q.LU = None
    for k, v in fields.items():
        setattr(q, k, v)
    from multigrid_jl_amd.mgsetup import defineCoarsestAinv
    defineCoarsestAinv(q, q.As[-1])
    return q


def _rounds(params, media, b, cycles=20):
    from multigrid_jl_amd.mgdef import _release_device
    rec = {k: dict(replace_plus_cycle_s=[], upload_plus_cycle_s=[], cycle_ms=[], parts=[]) for k in params}
    x = np.zeros_like(b)
    for k, p in params.items():                                 # resident, and one unrecorded replacement (transposed patterns)
        mg.recursiveCycle(p, b, x)
        mg.replaceMatrixInHierarchy(p, media[1])
    for r in range(ROUNDS):
        for k, p in params.items():
            A = media[r % 2]
            x[:] = 0
            dev = p.device

            def go():
                mg.replaceMatrixInHierarchy(p, A)
                mg.recursiveCycle(p, b, x)
            rec[k]["replace_plus_cycle_s"].append(timed(go)[0])
            assert p.device is dev
            t = {}
            if hasattr(dev, "rap_level_ms"):
                dev.replace_matrix(p, A, timings=t)
                rec[k]["parts"].append(t)
            ts = []
            for _ in range(cycles):
                x[:] = 0
                ts.append(timed(lambda: mg.recursiveCycle(p, b, x))[0] * 1e3)
            rec[k]["cycle_ms"].append(float(np.median(ts)))
            _release_device(p)
            x[:] = 0
            rec[k]["upload_plus_cycle_s"].append(timed(lambda: mg.recursiveCycle(p, b, x))[0])
    out = {}
    for k, v in rec.items():
        out[k] = {name: stats(v[name]) for name in ("replace_plus_cycle_s", "upload_plus_cycle_s", "cycle_ms")}
        if v["parts"]:
            out[k]["parts_median_s"] = {name: float(np.median([t[name] for t in v["parts"]])) for name in v["parts"][0]}
        out[k]["route_device"] = bool(params[k].device._coarse_device_inverse)
    return out


def part_hier():
    from complex_cases import complex_rhs
    cells = int(os.environ.get("CDI_CELLS", "128"))
    mesh = mg.getRegularMesh([0.0, 1.0] * 3, [cells] * 3)
    L = mg.getNodalLaplacianMatrix(mesh).tocsr().astype(np.complex128)
    n = L.shape[0]
    k2 = 0.25 * 0.25 * L.diagonal().real.max() / 6.0

    def operator(m):
        A = (L - sp.diags((1.0 - 0.5j) * k2 * m, format="csr")).tocsr()
        A.sort_indices()
        return A

    rng = np.random.default_rng(5)
    t0 = time.perf_counter()
    p = mg.getMGparam(np.complex128, np.int64, 4, 8, 10, 0.0, "SPAI", 1.0, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(operator(np.ones(n)), mesh, p)
    setup_s = time.perf_counter() - t0
    q = _copy_param(p, coarseDeviceInverse=True)
    media = [operator(0.8 + 0.2 * rng.random(n)) for _ in range(2)]
    t_splu = [timed(lambda: spla.splu(sp.csc_matrix(p.As[-1])))[0] for _ in range(3)]
    out = dict(cells=cells, rows=[int(M.shape[0]) for M in p.As], host_setup_s=setup_s, splu_coarsest_s=stats(t_splu))
    out.update(_rounds({"flag_off": p, "flag_on": q}, media, complex_rhs(n, 21)))
    return out


def part_vanka():
    import complex_vanka_cases as CV
    cells = int(os.environ.get("CDI_VANKA_CELLS", "64"))
    nn = [cells] * 3
    A = CV.operator(nn, 0.15)
    mk = lambda **kw: mg.getMGparam(np.complex128, np.int64, 4, 1, 3, 1e-30, "VankaFaces", CV.W, 1, 1, "V", "NoMUMPS", 0.4, 0.0,
                                    "SystemsFacesMixedLinear", complexVanka=True, vankaDeviceSetup=True, **kw)
    t0 = time.perf_counter()
    p = mk()
    mg.MGsetup(A, CV.mesh(mg, nn), p)
    setup_s = time.perf_counter() - t0
    q = _copy_param(p, coarseDeviceInverse=True)
    media = [sp.csr_matrix(A * (2 - 0.5j)), sp.csr_matrix(A * (1.5 - 0.25j))]
    out = dict(cells=cells, rows=[int(M.shape[0]) for M in p.As], host_setup_s=setup_s)
    out.update(_rounds({"flag_off": p, "flag_on": q}, media, CV.rhs(A.shape[0]), cycles=5))
    return out


def part_unchanged():
    from complex_cases import complex_rhs, helmholtz
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]
    out = dict(tree=os.path.abspath(args.root))

    def run(name, f, x):
        f()
        ts = []
        for _ in range(30):
            x[...] = 0
            ts.append(timed(f)[0] * 1e3)
        out[name] = dict(sha=sha(x), ms=stats(ts))

    A, mesh = helmholtz(mg, [64, 64, 64])
    p = mg.getMGparam(np.complex128, np.int64, 3, 1, 10, 1e-30, "Jac", 0.8, 2, 1, "V", "NoMUMPS", 0.4, 0.0)
    mg.MGsetup(A, mesh, p)
    b = complex_rhs(A.shape[0], 21)
    x = np.zeros_like(b)
    run("cf64_jac_cycle", lambda: mg.recursiveCycle(p, b, x), x)
    B = np.asfortranarray(np.stack([complex_rhs(A.shape[0], 30 + j) for j in range(4)], axis=1))
    X = np.zeros_like(B, order="F")
    run("cf64_block4_cycle", lambda: mg.to_device(p).block_cycle(B, X, 1), X)
    Lr = mg.getNodalLaplacianMatrix(mesh).tocsr()
    Ar = (Lr + sp.identity(Lr.shape[0], format="csr")).tocsr()
    Ar.sort_indices()
    pr = mg.getMGparam(np.float64, np.int64, 3, 1, 10, 1e-30, "Jac", 0.8, 2, 1, "V", "NoMUMPS", 0.4, 0.0)
    mg.MGsetup(Ar, mesh, pr)
    br = np.random.default_rng(3).standard_normal(Ar.shape[0])
    xr = np.zeros_like(br)
    run("fp64_jac_cycle", lambda: mg.recursiveCycle(pr, br, xr), xr)
    return out


result = {"standalone": part_standalone, "hier": part_hier, "vanka": part_vanka, "unchanged": part_unchanged}[args.part]()
print(json.dumps(result, indent=1))
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
