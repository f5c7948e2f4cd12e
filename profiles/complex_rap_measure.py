"""Measurements behind profiles/complex_rap.md (replaceMatrixInHierarchy of a ComplexF64 hierarchy on the device).
    python profiles/complex_rap_measure.py one [--root TREE] [--rounds N] [--groups G] [--out FILE.json]
    python profiles/complex_rap_measure.py all --parent TREE [--out FILE.json]
Problem: the hierarchy of profiles/complex_krylov.md (shifted Laplacian at 128^3 cells, k h = 0.25, damping 0.5, four levels, SPAI,
V(2,1)), resident after one cycle; then media on the same pattern, k^2 scaled point by point by a seeded factor in [0.8, 1].
one   times ONE tree in this process (--root names the tree whose package and built library are imported, so the parent commit is
      timed by the same script): an unrecorded first replacement (on this commit it builds the transposed patterns of SPAI's column
      sums, once per level), then N rounds of
        call        replaceMatrixInHierarchy(param, A_new), host clock
        call+cycle  the same plus the first following recursiveCycle from host vectors (the parent re-uploads the hierarchy there)
      and, where the tree has the device path, three more replacements for the split: device milliseconds per level by events
      (mg_rap_level_ms_CF64), seconds of mg_rap_CF64 as the host sees it (upload of the fine values included), of the readback and of
      the host's coarsest factorisation with its upload.  --groups G sets the option rap_groups (lane groups of cx_rap_numeric).
all   ROUNDS alternating rounds, each a fresh process per tree (parent, this commit, parent, ...), then the two forms of the kernel
      (rap_groups = 1: the walk of rap_numeric; 8: eight rows of A side by side), alternating as well; medians and spreads.
CR_CELLS overrides the 128 (rehearsals)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("part", choices=["one", "all"])
ap.add_argument("--root", default=HERE)
ap.add_argument("--parent", default=None)
ap.add_argument("--rounds", type=int, default=1)
ap.add_argument("--groups", type=int, default=0)
ap.add_argument("--out", default=None)
args = ap.parse_args()
CELLS = int(os.environ.get("CR_CELLS", "128"))
ROUNDS, SPLIT_REPS = 5, 3


def stats(v):
    import numpy as np
    v = np.asarray(v, dtype=float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(v.size))


def part_one():
    if args.groups:
        os.environ["MG_RAP_GROUPS"] = str(args.groups)
    sys.path.insert(0, os.path.abspath(args.root))
    sys.path.insert(1, os.path.join(HERE, "tests"))
    import torch  # noqa: F401  (first: it bundles its own HIP runtime)
    import numpy as np
    import scipy.sparse as sp
    import multigrid_jl_amd as mg
    from complex_cases import complex_rhs

    mesh = mg.getRegularMesh([0.0, 1.0] * 3, [CELLS] * 3)
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
    b = complex_rhs(n, 21)
    x = np.zeros_like(b)
    mg.recursiveCycle(p, b, x)                                      # uploads the hierarchy
    media = [operator(0.8 + 0.2 * rng.random(n)) for _ in range(2)]
    has_device_path = "mg_rap_CF64" in mg.device.SIGNATURES
    rec = dict(tree=os.path.abspath(args.root), cells=CELLS, rows=[int(M.shape[0]) for M in p.As], nnz=[int(M.nnz) for M in p.As],
               host_setup_s=setup_s, device_path=has_device_path, groups=args.groups, call_s=[], call_plus_cycle_s=[])

    def one_round(A):
        x[:] = 0
        dev = p.device
        t0 = time.perf_counter()
        mg.replaceMatrixInHierarchy(p, A)
        t1 = time.perf_counter()
        mg.recursiveCycle(p, b, x)
        t2 = time.perf_counter()
        return t1 - t0, t2 - t0, p.device is dev

    c, cc, kept = one_round(media[0])
    rec.update(first_call_s=c, first_call_plus_cycle_s=cc, device_kept=kept)
    for r in range(args.rounds):
        c, cc, kept = one_round(media[(r + 1) % 2])
        rec["call_s"].append(c)
        rec["call_plus_cycle_s"].append(cc)
        assert kept == has_device_path
    rec["x_norm"] = float(np.linalg.norm(x))                        # the same number from both trees: they compute the same thing
    if has_device_path:
        split = dict(level_ms=[], rap_s=[], readback_s=[], coarsest_s=[])
        for r in range(SPLIT_REPS):
            t = {}
            p.device.replace_matrix(p, media[r % 2], timings=t)
            split["level_ms"].append([float(v) for v in p.device.rap_level_ms()])
            split["rap_s"].append(t["rap"])
            split["readback_s"].append(t["readback"])
            split["coarsest_s"].append(t["coarsest"])
        rec["split"] = split
    mg.clear_(p)
    print("one", json.dumps(rec), flush=True)
    return rec


def child(root, groups=0):
    """One fresh process per sample: the trees cannot share one (the same package name, two libraries)."""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "one.json")
        cmd = [sys.executable, os.path.abspath(__file__), "one", "--root", root, "--rounds", "1", "--out", path]
        if groups:
            cmd += ["--groups", str(groups)]
        r = subprocess.run(cmd, timeout=300)
        if r.returncode != 0:
            sys.exit(f"the measurement of {root} ended with status {r.returncode}: nothing more is started")
        return json.load(open(path))


def part_all():
    if not args.parent:
        sys.exit("all needs --parent TREE (a built checkout of the parent commit)")
    runs = {"parent": [], "this": []}
    for r in range(ROUNDS):
        for name, root in (("parent", args.parent), ("this", HERE)) if r % 2 == 0 else (("this", HERE), ("parent", args.parent)):
            runs[name].append(child(root))
    res = dict(cells=CELLS, rounds=ROUNDS)
    for name, rs in runs.items():
        res[name] = dict(rows=rs[0]["rows"], nnz=rs[0]["nnz"], device_kept=[r["device_kept"] for r in rs],
                         call_s=stats([v for r in rs for v in r["call_s"]]),
                         call_plus_cycle_s=stats([v for r in rs for v in r["call_plus_cycle_s"]]),
                         first_call_s=stats([r["first_call_s"] for r in rs]), x_norm=[r["x_norm"] for r in rs])
    this = runs["this"]
    res["this"]["split"] = dict(
        level_ms=[stats([s[l] for r in this for s in r["split"]["level_ms"]]) for l in range(len(this[0]["rows"]) - 1)],
        rap_s=stats([v for r in this for v in r["split"]["rap_s"]]),
        readback_s=stats([v for r in this for v in r["split"]["readback_s"]]),
        coarsest_s=stats([v for r in this for v in r["split"]["coarsest_s"]]))
    forms = {1: [], 8: []}
    for r in range(ROUNDS):
        for g in (1, 8) if r % 2 == 0 else (8, 1):
            forms[g].append(child(HERE, g))
    res["kernel_forms"] = {
        f"groups_{g}": dict(level_ms=[stats([s[l] for r in rs for s in r["split"]["level_ms"]]) for l in range(len(rs[0]["rows"]) - 1)],
                            total_ms=stats([sum(s) for r in rs for s in r["split"]["level_ms"]]))
        for g, rs in forms.items()}
    print("all", json.dumps(res), flush=True)
    return res


res = {"one": part_one, "all": part_all}[args.part]()
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)
