"""Measurements behind profiles/complex_single_rap.md (replaceMatrixInHierarchy of a ComplexF32 hierarchy on the device).
    python profiles/complex_single_rap_measure.py single [--out FILE.json]
    python profiles/complex_single_rap_measure.py vanka  [--out FILE.json]
    python profiles/complex_single_rap_measure.py regress [--out FILE.json]      (run once per tree: --root TREE)
single   the hierarchy of profiles/complex_rap.md (shifted Laplacian at 128^3 cells, k h = 0.25, damping 0.5, four levels, SPAI,
         V(2,1)) with singlePrecision=True, set up once on the host; per coarsest-solve configuration (coarseDeviceInverse, GMRES, the
         default host inverse) two params on that hierarchy, one with singleDeviceSetup and one without (the parent commit's route: host
         products, the device copy dropped, the upload by the next cycle), both resident; an unrecorded first replacement each, then
         ROUNDS rounds alternating between the two and between two media of
             call        replaceMatrixInHierarchy(param, A_new), host clock
             call+cycle  the same plus the first following recursiveCycle from host vectors (ends in a device synchronisation)
         then three more replacements on the device route for the split (timings of replace_matrix, mg_rap_level_ms_CF32), and the
         same three on a ComplexF64 param of the same grid (mg_rap_level_ms_CF64).
vanka    the same pair on the 64^3 four-level single VankaFaces hierarchy of profiles/vanka_device_setup.md, if it sets up.
regress  what exists, for a comparison between two trees (--root names the tree whose package and library are imported): device time
         by events of the ComplexF64 V(2,1) Jac cycle, the 4-column block cycle and the ComplexF32 V(2,1) cycle at 64^3, the ComplexF64
         replaceMatrixInHierarchy + first cycle with coarseDeviceInverse at 128^3, and a checksum of every result.
CSR_CELLS overrides the 128 (rehearsals)."""
import argparse
import hashlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("part", choices=["single", "vanka", "regress"])
ap.add_argument("--root", default=HERE)
ap.add_argument("--out", default=None)
args = ap.parse_args()
CELLS = int(os.environ.get("CSR_CELLS", "128"))
ROUNDS, SPLIT_REPS = 5, 3
sys.path.insert(0, os.path.abspath(args.root))
sys.path.insert(1, os.path.join(HERE, "tests"))
import torch  # noqa: E402,F401  (first: it bundles its own HIP runtime)
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import multigrid_jl_amd as mg  # noqa: E402
from complex_cases import complex_rhs, helmholtz  # noqa: E402


def stats(v):
    v = np.asarray(v, dtype=float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(v.size))


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def clone(p, **kw):
    """A param on p's hierarchy (operators copied: a replacement writes them in place) with other keyword flags; its coarsest solve
    set up by defineCoarsestAinv."""
    from multigrid_jl_amd.mgsetup import defineCoarsestAinv
    coarse = kw.pop("coarse", "NoMUMPS")
    q = mg.getMGparam(np.complex128, np.int64, p.levels, 8, 10, 0.0, p.relaxType, p.relaxParam, 2, 1, "V", coarse, 0.5, 0.0,
                      p.transferOperatorType, singlePrecision=bool(p.singlePrecision), **kw)
    q.As = [M.copy() for M in p.As]
    q.Ps, q.Rs, q.Meshes = list(p.Ps), list(p.Rs), list(p.Meshes)
    q.relaxPrecs = [np.array(d, copy=True) for d in p.relaxPrecs]
    q.levels, q.nrhs = p.levels, 1
    defineCoarsestAinv(q, q.As[-1])
    return q


def pair_rounds(pf, ph, mats, b, tag):
    """ROUNDS alternating rounds of (pf: the device route, ph: the host route): call and call + first cycle, seconds."""
    rec = {k: dict(call_s=[], call_plus_cycle_s=[], kept=[]) for k in ("device", "host")}
    x = np.zeros_like(b)

    def one(p, A):
        x[:] = 0
        dev = p.device
        t0 = time.perf_counter()
        mg.replaceMatrixInHierarchy(p, A)
        t1 = time.perf_counter()
        mg.recursiveCycle(p, b, x)
        t2 = time.perf_counter()
        return t1 - t0, t2 - t0, p.device is dev

    for name, p in (("device", pf), ("host", ph)):                  # unrecorded: the transposed patterns of SPAI, first launches
        mg.recursiveCycle(p, b, x)
        one(p, mats[0])
    for r in range(ROUNDS):
        order = (("device", pf), ("host", ph)) if r % 2 == 0 else (("host", ph), ("device", pf))
        for name, p in order:
            c, cc, kept = one(p, mats[(r + 1) % 2])
            rec[name]["call_s"].append(c)
            rec[name]["call_plus_cycle_s"].append(cc)
            rec[name]["kept"].append(bool(kept))
            rec[name]["x_norm"] = float(np.linalg.norm(x.astype(np.complex128)))
            print(f"{tag} round {r} {name}: call {c:.3f} s, call + cycle {cc:.3f} s, handle kept {kept}", flush=True)
    out = {}
    for name, v in rec.items():
        out[name] = dict(call_s=stats(v["call_s"]), call_plus_cycle_s=stats(v["call_plus_cycle_s"]), kept=v["kept"], x_norm=v["x_norm"])
    return out


def split_of(p, mats):
    s = dict(level_ms=[], rap_s=[], readback_s=[], coarsest_s=[], blocks_readback_s=[])
    for r in range(SPLIT_REPS):
        t = {}
        p.device.replace_matrix(p, mats[r % 2], timings=t)
        s["level_ms"].append([float(v) for v in p.device.rap_level_ms()])
        s["rap_s"].append(t["rap"])
        s["readback_s"].append(t["readback"])
        s["coarsest_s"].append(t["coarsest"])
        s["blocks_readback_s"].append(t.get("blocks_readback", 0.0))
    nl = len(s["level_ms"][0])
    return dict(level_ms=[stats([v[l] for v in s["level_ms"]]) for l in range(nl)], rap_s=stats(s["rap_s"]),
                readback_s=stats(s["readback_s"]), coarsest_s=stats(s["coarsest_s"]), blocks_readback_s=stats(s["blocks_readback_s"]))


def laplacian_media(cells):
    mesh = mg.getRegularMesh([0.0, 1.0] * 3, [cells] * 3)
    L = mg.getNodalLaplacianMatrix(mesh).tocsr().astype(np.complex128)
    n = L.shape[0]
    k2 = 0.25 * 0.25 * L.diagonal().real.max() / 6.0

    def operator(m):
        A = (L - sp.diags((1.0 - 0.5j) * k2 * m, format="csr")).tocsr()
        A.sort_indices()
        return A

    rng = np.random.default_rng(5)
    return mesh, n, operator, [operator(0.8 + 0.2 * rng.random(n)) for _ in range(2)]


def part_single():
    mesh, n, operator, media = laplacian_media(CELLS)
    t0 = time.perf_counter()
    base = mg.getMGparam(np.complex128, np.int64, 4, 8, 10, 0.0, "SPAI", 1.0, 2, 1, "V", "NoMUMPS", 0.5, 0.0, singlePrecision=True)
    mg.MGsetup(operator(np.ones(n)), mesh, base)
    res = dict(cells=CELLS, rounds=ROUNDS, rows=[int(M.shape[0]) for M in base.As], nnz=[int(M.nnz) for M in base.As],
               host_setup_s=time.perf_counter() - t0, configs={})
    print(f"single: host setup {res['host_setup_s']:.1f} s, rows {res['rows']}", flush=True)
    b = complex_rhs(n, 21).astype(np.complex64)
    media32 = [M.astype(np.complex64) for M in media]
    for tag, kw in (("device_inverse", dict(coarseDeviceInverse=True)), ("gmres", dict(coarse="GMRES")), ("host_inverse", {})):
        pf, ph = clone(base, singleDeviceSetup=True, **kw), clone(base, **kw)
        r = pair_rounds(pf, ph, media32, b, tag)
        assert all(r["device"]["kept"]) and not any(r["host"]["kept"])
        r["split"] = split_of(pf, media32)
        res["configs"][tag] = r
        print(tag, json.dumps(r), flush=True)
        mg.clear_(pf)
        mg.clear_(ph)
    mg.clear_(base)
    # the ComplexF64 twin on the same grid: device milliseconds per level of mg_rap_CF64
    pd = mg.getMGparam(np.complex128, np.int64, 4, 8, 10, 0.0, "SPAI", 1.0, 2, 1, "V", "NoMUMPS", 0.5, 0.0, coarseDeviceInverse=True)
    mg.MGsetup(operator(np.ones(n)), mesh, pd)
    b64 = complex_rhs(n, 21)
    mg.recursiveCycle(pd, b64, np.zeros_like(b64))
    mg.replaceMatrixInHierarchy(pd, media[0])
    res["cf64_split"] = split_of(pd, media)
    print("cf64", json.dumps(res["cf64_split"]), flush=True)
    mg.clear_(pd)
    return res


def part_vanka():
    import vanka_cases as V
    cells = int(os.environ.get("CSR_VANKA_CELLS", "64"))
    t0 = time.perf_counter()
    A = V.mixed_operator([cells] * 3, True, omega=0.15)
    mats = [sp.csr_matrix(A * (2 - 0.5j)).astype(np.complex64), sp.csr_matrix(A).astype(np.complex64)]
    mesh = mg.getRegularMesh([0, 1] * 3, [cells] * 3)
    b = V.seeded(A.shape[0], 5, cx=True).astype(np.complex64)
    ps = []
    for kw in (dict(singleDeviceSetup=True), {}):
        p = mg.getMGparam(np.complex128, np.int64, 4, 1, 1, 1e-8, "VankaFaces", 0.6, 1, 1, "V", "NoMUMPS", 0.4, 0.0,
                          "SystemsFacesMixedLinear", singlePrecision=True, complexVanka=True, vankaDeviceSetup=True, **kw)
        mg.MGsetup(A, mesh, p)
        ps.append(p)
        print(f"vanka: set-up of one param done {time.perf_counter() - t0:.1f} s after the start, rows {[int(M.shape[0]) for M in p.As]}", flush=True)
    res = dict(cells=cells, rows=[int(M.shape[0]) for M in ps[0].As], setup_s=time.perf_counter() - t0)
    res.update(pair_rounds(ps[0], ps[1], mats, b, "vanka"))
    res["split"] = split_of(ps[0], mats)
    for p in ps:
        mg.clear_(p)
    return res


def event_ms(fn, reps):
    """median, min, max device milliseconds of fn() over reps calls, by events on the library's work (device synchronised around)."""
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return stats(ts)


def part_regress():
    res = dict(tree=os.path.abspath(args.root))
    cells = int(os.environ.get("CSR_REGRESS_CELLS", "64"))
    Ah, mesh = helmholtz(mg, [cells] * 3, 0.25, 0.5)
    n = Ah.shape[0]
    pj = mg.getMGparam(np.complex128, np.int64, 4, 8, 200, 1e-8, "Jac", 0.8, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(Ah, mesh, pj)
    ps = mg.getMGparam(np.complex128, np.int64, 4, 8, 200, 1e-8, "Jac", 0.8, 2, 1, "V", "NoMUMPS", 0.5, 0.0, singlePrecision=True)
    mg.MGsetup(Ah, mesh, ps)
    dj, ds = mg.device.DeviceHierarchy(pj), mg.device.DeviceHierarchy(ps)
    b = torch.from_numpy(complex_rhs(n, 21)).cuda()
    x = torch.zeros_like(b)
    B = torch.from_numpy(np.ascontiguousarray(np.stack([complex_rhs(n, 30 + j) for j in range(4)], axis=1))).cuda()
    X = torch.zeros_like(B)
    for name, fn, out in (("cf64_cycle", lambda: dj.cycle_dev(b, x, 1), x), ("cf64_block4_cycle", lambda: dj.block_cycle_dev(B, X, 1), X),
                          ("cf32_cycle", lambda: ds.cycle_dev(b, x, 1), x)):
        for _ in range(5):
            fn()
        res[name] = dict(ms=event_ms(fn, 50), bits=digest(out.cpu().numpy()))
        print(name, json.dumps(res[name]), flush=True)
    dj.close()
    ds.close()
    # ComplexF64 replaceMatrixInHierarchy + first cycle with coarseDeviceInverse
    meshL, nL, operator, media = laplacian_media(CELLS)
    pd = mg.getMGparam(np.complex128, np.int64, 4, 8, 10, 0.0, "SPAI", 1.0, 2, 1, "V", "NoMUMPS", 0.5, 0.0, coarseDeviceInverse=True)
    mg.MGsetup(operator(np.ones(nL)), meshL, pd)
    bL = complex_rhs(nL, 21)
    xL = np.zeros_like(bL)
    mg.recursiveCycle(pd, bL, xL)
    mg.replaceMatrixInHierarchy(pd, media[0])
    ts = []
    for r in range(ROUNDS):
        xL[:] = 0
        t0 = time.perf_counter()
        mg.replaceMatrixInHierarchy(pd, media[(r + 1) % 2])
        mg.recursiveCycle(pd, bL, xL)
        ts.append(time.perf_counter() - t0)
    res["cf64_resetup_plus_cycle"] = dict(s=stats(ts), bits=digest(xL), coarse_bits=digest(pd.As[-1].data))
    print("cf64_resetup_plus_cycle", json.dumps(res["cf64_resetup_plus_cycle"]), flush=True)
    mg.clear_(pd)
    return res


res = {"single": part_single, "vanka": part_vanka, "regress": part_regress}[args.part]()
print(args.part, json.dumps(res), flush=True)
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)
