"""adjointHierarchy of complex hierarchies on the device: what profiles/complex_adjoint.md reports.
    python profiles/complex_adjoint_measure.py all [out.json]
        128^3 cells, four levels, SPAI, with the GMRES coarsest solve and with the dense inverse.  Per round, alternating:
          flip       adjointHierarchy of the resident hierarchy plus the first following cycle, split into the host mirror (scipy's
                     conjugate transposes, splu of the coarsest adjoint) and mg_adjoint_hierarchy_CF64; the library prints the device time
                     per level on stderr (option debug_format)
          re-setup   the only route without it: MGsetup on A' of a fresh param, the upload, the first cycle
        and the byte model of one operator's adjoint against the time the library reports for it.
    python profiles/complex_adjoint_measure.py baseline [out.json]
        the re-setup route alone, REPS rounds per coarsest solve - run with MGVCYCLE_LIB naming the parent commit's library
    python profiles/complex_adjoint_measure.py regress OTHER_LIB [out.json]
        what exists: the V(2,1) Jac cycle with the dense inverse and the 4-column block cycle of THIS tree's library against another
        build of libmgvcycle.so (the parent commit's), one child process each, rounds alternating between the two
    python profiles/complex_adjoint_measure.py rehearse
        everything the above builds on the host, at 16^3 cells, without a device
Times are wall-clock around work that ends in a device synchronisation, medians of REPS rounds with min and max as the spread.
ADJ_CELLS overrides the 128 (rehearsals)."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CELLS = int(os.environ.get("ADJ_CELLS", "128"))
REPS, WARM = 5, 1
NEW_SYMBOLS = ("mg_adjoint_hierarchy_CF64", "mg_adjoint_hierarchy_CF32")


def stat(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def fmt(v, unit="s"):
    return f"{np.median(v):.3f} {unit} [{min(v):.3f}, {max(v):.3f}]"


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def operator(mg, cells=None):
    """The shifted Laplacian with a one-sided complex perturbation: non-symmetric, non-Hermitian (the tests' base operator)."""
    from complex_adjoint_cases import base_operator
    return base_operator(mg, [cells or CELLS] * 3)


def new_param(mg, relax, coarse):
    return mg.getMGparam(np.complex128, np.int64, 4, 8, 200, 1e-8, relax, 0.8 if relax == "Jac" else 1.0, 2, 1, "V", coarse, 0.5, 0.0)


def resetup_route(mg, torch, At, mesh, coarse, b):
    """MGsetup on A' of a fresh param, upload, first cycle: seconds of (setup, upload + cycle)."""
    p = new_param(mg, "SPAI", coarse)
    t0 = time.perf_counter()
    mg.MGsetup(At, mesh, p)
    t1 = time.perf_counter()
    x = np.zeros_like(b)
    sec = timed(torch, lambda: mg.recursiveCycle(p, b, x, 1))[0]
    mg.clear_(p)
    return t1 - t0, sec


def byte_model(M):
    """Least bytes the three kernels move for one complex operator of nnz entries, n rows and m columns (segments re-read by the
    ranking and the bisected row pointers are taken as cached: counted once)."""
    n, m = M.shape
    nnz = M.nnz
    count = 4 * nnz + 4 * m                                   # column indices read, counters updated
    scatter = 4 * nnz + 4 * (n + 1) + 4 * (m + 1) + 4 * m + 4 * nnz      # indices, both pointer arrays, cursors, row indices written
    order = (4 + 16) * nnz + 4 * (n + 1) + 4 * (m + 1) + 4 * nnz + (4 + 16) * nnz   # indices + values read, segments read, result written
    return count + scatter + order


def measure_all(mg, torch, out):
    from complex_cases import complex_rhs
    A, mesh = operator(mg)
    At = A.conj().T.tocsr()
    At.sort_indices()
    b = complex_rhs(A.shape[0], 21)
    ps = {}
    for coarse in ("GMRES", "NoMUMPS"):
        p = new_param(mg, "SPAI", coarse)
        t0 = time.perf_counter()
        mg.MGsetup(A, mesh, p)
        t1 = time.perf_counter()
        sec = timed(torch, lambda: mg.recursiveCycle(p, b, np.zeros_like(b), 1))[0]
        assert p.device.lib.mg_set_option(p.device.handle, b"debug_format", 1.0) == 0
        print(f"{CELLS}^3 {coarse}: MGsetup {t1 - t0:.2f} s, upload + first cycle {sec:.2f} s, levels {[M.shape[0] for M in p.As]}", flush=True)
        ps[coarse] = p
    out["byte_model"] = {f"As[{l + 1}]": dict(nnz=int(M.nnz), rows=int(M.shape[0]), bytes=int(byte_model(M))) for l, M in enumerate(ps["GMRES"].As)}
    t = {c: dict(total=[], host=[], device=[], cycle=[], resetup=[], resetup_setup=[], resetup_upload=[]) for c in ps}
    for rep in range(WARM + REPS):
        for coarse, p in ps.items():
            dev = p.device
            spent = {}
            inner = dev.adjoint_hierarchy

            def wrapped(param, inner=inner, spent=spent):
                spent["device"] = timed(torch, lambda: inner(param))[0]

            dev.adjoint_hierarchy = wrapped
            print(f"-- round {rep} {coarse}: flip", file=sys.stderr, flush=True)
            t_flip = timed(torch, lambda: mg.adjointHierarchy(p))[0]
            del dev.adjoint_hierarchy
            assert p.device is dev
            x = np.zeros_like(b)
            t_cyc = timed(torch, lambda: mg.recursiveCycle(p, b, x, 1))[0]
            s_setup, s_up = resetup_route(mg, torch, At, mesh, coarse, b)
            if rep >= WARM:
                r = t[coarse]
                r["total"].append(t_flip + t_cyc); r["host"].append(t_flip - spent["device"]); r["device"].append(spent["device"])
                r["cycle"].append(t_cyc); r["resetup"].append(s_setup + s_up); r["resetup_setup"].append(s_setup); r["resetup_upload"].append(s_up)
    for coarse, r in t.items():
        out[coarse] = {k: stat(v) for k, v in r.items()}
        print(f"{coarse}: adjointHierarchy + first cycle {fmt(r['total'])} = host mirror {fmt(r['host'])} + mg_adjoint_hierarchy_CF64 {fmt(r['device'])} "
              f"+ cycle {fmt(r['cycle'])};  MGsetup(A') + upload + first cycle {fmt(r['resetup'])} = {fmt(r['resetup_setup'])} + {fmt(r['resetup_upload'])}",
              flush=True)
    for p in ps.values():
        mg.clear_(p)


def baseline(out):
    import torch
    import multigrid_jl_amd as mg
    if os.environ.get("ADJ_OTHER") == "1":
        for k in NEW_SYMBOLS:
            mg.device.SIGNATURES.pop(k, None)
    from complex_cases import complex_rhs
    A, mesh = operator(mg)
    At = A.conj().T.tocsr()
    At.sort_indices()
    b = complex_rhs(A.shape[0], 21)
    for coarse in ("GMRES", "NoMUMPS"):
        ts = []
        for rep in range(WARM + REPS):
            s = resetup_route(mg, torch, At, mesh, coarse, b)
            if rep >= WARM:
                ts.append(s)
        out[coarse] = dict(total=stat([a + c for a, c in ts]), setup=stat([a for a, _ in ts]), upload_cycle=stat([c for _, c in ts]))
        print(f"baseline {coarse} ({os.environ.get('MGVCYCLE_LIB', 'this tree')}): MGsetup(A') + upload + first cycle {fmt([a + c for a, c in ts])} "
              f"= {fmt([a for a, _ in ts])} + {fmt([c for _, c in ts])}", flush=True)


def child():
    """One process on the library named by MGVCYCLE_LIB: REPS rounds of the two existing cycles, printed as JSON."""
    import torch
    import multigrid_jl_amd as mg
    if os.environ.get("ADJ_OTHER") == "1":
        for k in NEW_SYMBOLS:
            mg.device.SIGNATURES.pop(k, None)
    from complex_cases import complex_rhs, helmholtz
    Ah, mesh = helmholtz(mg, [CELLS] * 3, 0.25, 0.5)
    p = new_param(mg, "Jac", "NoMUMPS")
    mg.MGsetup(Ah, mesh, p)
    n = Ah.shape[0]
    dev = mg.device.DeviceHierarchy(p)
    bt = torch.from_numpy(complex_rhs(n, 21)).cuda()
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
    import hashlib
    digest = hashlib.sha256(xt.cpu().numpy().tobytes() + Xt.cpu().numpy().tobytes()).hexdigest()
    print("RESULT " + json.dumps(dict(vcycle_ms=tv, block4_ms=tb, digest=digest)), flush=True)
    dev.close()


def regress(other_lib, out_path):
    """Two child processes per library, alternating: this, other, this, other."""
    res = {"this": dict(vcycle_ms=[], block4_ms=[]), "other": dict(vcycle_ms=[], block4_ms=[])}
    digests = {}
    for rnd in range(2):
        for which in ("this", "other"):
            env = dict(os.environ)
            if which == "other":
                env["MGVCYCLE_LIB"], env["ADJ_OTHER"] = os.path.abspath(other_lib), "1"
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-2000:])
                sys.exit(p.returncode)
            r = json.loads([ln for ln in p.stdout.split("\n") if ln.startswith("RESULT ")][0][7:])
            for k in ("vcycle_ms", "block4_ms"):
                res[which][k] += r[k]
            digests[which] = r["digest"]
    out = {w: {k: stat(v) for k, v in d.items()} for w, d in res.items()}
    out["same_bits"] = digests["this"] == digests["other"]
    for k in ("vcycle_ms", "block4_ms"):
        print(f"{k}: this {fmt(res['this'][k], 'ms')}   other {fmt(res['other'][k], 'ms')}")
    print("same bits of x (vector cycle and 4-column block cycle):", out["same_bits"])
    if out_path:
        json.dump(out, open(out_path, "w"), indent=1)


def rehearse():
    import multigrid_jl_amd as mg
    A, mesh = operator(mg, 16)
    for coarse in ("GMRES", "NoMUMPS"):
        p = new_param(mg, "SPAI", coarse)
        mg.MGsetup(A, mesh, p)
        mg.adjointHierarchy(p)
        print(coarse, [M.shape[0] for M in p.As], type(p.LU).__name__, {f"As[{l + 1}]": byte_model(M) for l, M in enumerate(p.As)})


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    if mode == "rehearse":
        rehearse()
    elif mode == "child":
        child()
    elif mode == "regress":
        regress(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        out = dict(cells=CELLS, reps=REPS)
        if mode == "baseline":
            baseline(out)
        else:
            import torch
            import multigrid_jl_amd as mg
            measure_all(mg, torch, out)
        if len(sys.argv) > 2:
            json.dump(out, open(sys.argv[2], "w"), indent=1)
