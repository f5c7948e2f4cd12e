"""The device set-up of the Vanka cell blocks (vanka_build_blocks, csrc/mg_vanka.hpp): what profiles/vanka_device_setup.md reports.
    python profiles/vanka_device_setup_measure.py build CELLS [out.json]
        the build kernel on the stand-alone handle, the mixed 3-D operator of tests/vanka_cases.py on CELLS^3 cells with pressure
        (block size 7), FULL_VANKA_RB with the pair (0.6, 0.4) (the full blocks), ComplexF64 and FP64: device ms of one build
        (mg_vanka_time_build: events around the launch), the bytes of its byte model (the cells' operator rows read - values,
        int32 columns, two row pointers per row - and the blocks written) and the host function's seconds in the same job
        (VDS_HOST_REPS rounds, default 5)
    python profiles/vanka_device_setup_measure.py resetup [out.json]
        replaceMatrixInHierarchy plus the first following cycle on VDS_CELLS^3 cells (default 64), four levels, ComplexF64 VankaFaces
        w = 0.6: a param with vankaDeviceSetup=True (operators and blocks refreshed in HBM) against a default complex Vanka param
        (host recompute, the handle dropped and uploaded again by the cycle), rounds alternating; the `timings` split and the
        per-level device ms of mg_rap_CF64
    python profiles/vanka_device_setup_measure.py regress OTHER_LIB [out.json]
        what exists, THIS tree's library against another build of libmgvcycle.so (the parent commit's), one child process each,
        rounds alternating: the FP64 Vanka V(1,1) cycle, the ComplexF64 one-vector Vanka V(1,1) cycle and the 4-column Jac block
        cycle; the bits of their results are compared
    python profiles/vanka_device_setup_measure.py rehearse
        the host side of the above at 8^3 cells, without a device
Device times are medians of 5 rounds in which the variants alternate, with min and max as the spread."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

from complex_vanka_measure import BATCH, MIXED, OMEGA, REPS, WARM, digest, fmt, stat, timed, vanka_param   # noqa: E402

W_PAIR = (0.6, 0.4)
NEW_SYMBOLS = ("mg_vanka_create_built_FP64_INT64", "mg_vanka_create_built_CFP64_INT64", "mg_vanka_build_blocks_FP64",
               "mg_vanka_build_blocks_CFP64", "mg_vanka_replace_values_FP64", "mg_vanka_replace_values_CFP64", "mg_vanka_get_blocks",
               "mg_vanka_time_build", "mg_build_vanka_CF64", "mg_build_vanka_CF32", "mg_get_vanka_blocks_CF64", "mg_get_vanka_blocks_CF32")


def byte_model(mg, A, n):
    """(bytes read, bytes written) of one build: every row of every cell once, and the cell's bs*bs single-precision values."""
    from multigrid_jl_amd.vanka import _all_cell_indices, getVankaBlockSize
    bs, nf = getVankaBlockSize(np.asarray(n), True)
    I = _all_cell_indices(np.asarray(n), nf, True) - 1
    rowlen = np.diff(A.indptr)
    vs = 16 if np.iscomplexobj(A.data) else 8
    read = int((rowlen[I] * (vs + 4) + 8).sum())
    written = int(I.shape[0]) * bs * bs * (8 if vs == 16 else 4)
    return read, written


def build(cells, out_path):
    import multigrid_jl_amd as mg
    import vanka_cases as V
    lib = mg.device.load_library()
    n = [cells] * 3
    host_reps = int(os.environ.get("VDS_HOST_REPS", "5"))
    out = dict(cells=cells, kinds={})
    handles, w = {}, np.array(W_PAIR)
    for kind, omega in (("cf64", OMEGA), ("fp64", None)):
        t0 = time.perf_counter()
        A = V.mixed_operator(n, True, omega=omega)
        print(f"{kind}: {cells}^3 cells, {A.shape[0]} unknowns, {A.nnz} non-zeros (built in {time.perf_counter() - t0:.1f} s)", flush=True)
        read, written = byte_model(mg, A, n)
        host = []
        for _ in range(host_reps):
            t0 = time.perf_counter()
            Dh = mg.setupVankaFacesPreconditioner(A, np.asarray(n), W_PAIR, True, V.FULL_VANKA_RB)
            host.append(time.perf_counter() - t0)
        handles[kind] = mg.vanka.vanka_handle(A, None, n, True, w=W_PAIR, VankaType=V.FULL_VANKA_RB)
        Dd = handles[kind].blocks()
        bd, bh = Dd.T.view(np.uint32), Dh.T.view(np.uint32)       # (column-major blocks: the transposes are contiguous)
        diff = float(np.count_nonzero(bd != bh)) / bd.size
        out["kinds"][kind] = dict(unknowns=int(A.shape[0]), nnz=int(A.nnz), read=read, written=written, host_s=stat(host),
                                  bits_differ_share=diff, max_abs_diff=float(np.abs(Dd - Dh).max()))
        print(f"  host function {fmt(stat(host))} s; byte model {read / 1e9:.3f} GB read + {written / 1e9:.3f} GB written; "
              f"device blocks differ from the host's in {diff:.2e} of the components (max |diff| {np.abs(Dd - Dh).max():.2e})", flush=True)
        del A, Dh, Dd
    ms = {k: [] for k in handles}
    one = np.zeros(3)
    for rnd in range(WARM + REPS):
        for k, H in handles.items():
            mg.device._check(lib, lib.mg_vanka_time_build(H.h, V.FULL_VANKA_RB, w.ctypes.data_as(C.POINTER(C.c_double)), 2, 1, 3,
                                                          one.ctypes.data_as(C.POINTER(C.c_double))), "mg_vanka_time_build")
            if rnd >= WARM:
                ms[k].append(float(np.median(one)))
    for k, H in handles.items():
        r = out["kinds"][k]
        r["build_ms"] = stat(ms[k])
        r["gb_per_s"] = (r["read"] + r["written"]) / 1e9 / (r["build_ms"]["median"] / 1e3)
        print(f"{k}: build {fmt(r['build_ms'])} ms  = {r['gb_per_s']:.0f} GB/s of the byte model; host / device = "
              f"{r['host_s']['median'] * 1e3 / r['build_ms']['median']:.0f}x", flush=True)
        H.close()
    if out_path:
        json.dump(out, open(out_path, "w"), indent=1)


def resetup(out_path):
    import torch
    import multigrid_jl_amd as mg
    import vanka_cases as V
    cells = int(os.environ.get("VDS_CELLS", "64"))
    A = V.mixed_operator([cells] * 3, True, omega=OMEGA)
    mats = [(A * (2 - 0.5j)).tocsr(), A]
    b = V.seeded(A.shape[0], 5, cx=True)
    mesh = mg.getRegularMesh([0, 1] * 3, [cells] * 3)
    params, setup_s = {}, {}
    for name, kw in (("device", dict(vankaDeviceSetup=True)), ("host", {})):
        p = mg.getMGparam(np.complex128, np.int64, 4, 1, 1, 1e-8, "VankaFaces", 0.6, 1, 1, "V", "NoMUMPS", 0.4, 0.0, MIXED,
                          complexVanka=True, **kw)
        t0 = time.perf_counter()
        mg.MGsetup(A, mesh, p)
        x = np.zeros_like(b)
        mg.recursiveCycle(p, b, x)
        setup_s[name] = time.perf_counter() - t0
        params[name] = p
    print(f"{cells}^3 cells, levels {[int(M.shape[0]) for M in params['host'].As]}; MGsetup + upload + first cycle: "
          + "  ".join(f"{k} {v:.2f} s" for k, v in setup_s.items()), flush=True)
    t = {k: [] for k in params}
    xs = {}
    for rnd in range(WARM + REPS):
        for k, p in params.items():
            x = np.zeros_like(b)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mg.replaceMatrixInHierarchy(p, mats[rnd % 2])
            mg.recursiveCycle(p, b, x)
            torch.cuda.synchronize()
            if rnd >= WARM:
                t[k].append(time.perf_counter() - t0)
            xs[k] = x
    out = dict(cells=cells, setup_s=setup_s, resetup_plus_cycle_s={k: stat(v) for k, v in t.items()},
               x_distance=float(np.abs(xs["device"] - xs["host"]).max() / np.abs(xs["host"]).max()))
    split = {}
    params["device"].device.replace_matrix(params["device"], mats[0], timings=split)
    out["timings"] = split
    out["rap_level_ms"] = [float(v) for v in params["device"].device.rap_level_ms()]
    for k, s in out["resetup_plus_cycle_s"].items():
        print(f"replaceMatrixInHierarchy + first cycle, {k}: {fmt(s)} s", flush=True)
    print("timings of the device route: " + "  ".join(f"{k} {v * 1e3:.1f} ms" for k, v in split.items())
          + f";  mg_rap_CF64 per level (blocks + product) {np.round(out['rap_level_ms'], 3)} ms;  x of the two routes differ by "
          f"{out['x_distance']:.2e} of max|x|", flush=True)
    if out_path:
        json.dump(out, open(out_path, "w"), indent=1)


def child():
    import torch
    import multigrid_jl_amd as mg
    if os.environ.get("CV_OTHER") == "1":
        for k in NEW_SYMBOLS:
            mg.device.SIGNATURES.pop(k, None)
    import vanka_cases as V
    from complex_cases import complex_rhs, helmholtz
    cells = int(os.environ.get("VDS_CELLS", "64"))
    pr = vanka_param(mg, V.mixed_operator([cells] * 3, True), cells, np.float64)
    pc = vanka_param(mg, V.mixed_operator([cells] * 3, True, omega=OMEGA), cells, np.complex128)
    Ah, mesh = helmholtz(mg, [cells] * 3, 0.25, 0.5)
    pj = mg.getMGparam(np.complex128, np.int64, 4, 8, 200, 1e-8, "Jac", 0.8, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(Ah, mesh, pj)
    dv, dc, dj = (mg.device.DeviceHierarchy(q) for q in (pr, pc, pj))
    br = torch.from_numpy(V.seeded(pr.As[0].shape[0], 5)).cuda()
    xr = torch.zeros_like(br)
    bc = torch.from_numpy(V.seeded(pc.As[0].shape[0], 5, cx=True)).cuda()
    xc = torch.zeros_like(bc)
    bj = torch.from_numpy(complex_rhs(Ah.shape[0], 21)).cuda()
    Bj = torch.stack([bj, 2 * bj, 3 * bj, 4 * bj], dim=1).contiguous()
    Xj = torch.zeros_like(Bj)
    variants = {"fp64_vanka_v": lambda: dv.cycle_dev(br, xr, 1), "cf64_vanka_v": lambda: dc.cycle_dev(bc, xc, 1),
                "cf64_jac_block4": lambda: dj.block_cycle_dev(Bj, Xj, 1)}
    t = {k: [] for k in variants}
    for rep in range(WARM + REPS):
        for k, fn in variants.items():
            sec = timed(torch, lambda: [fn() for _ in range(BATCH)])[0]
            if rep >= WARM:
                t[k].append(1e3 * sec / BATCH)
    bits = dict(fp64_vanka_v=digest(xr.cpu().numpy()), cf64_vanka_v=digest(xc.cpu().numpy()), cf64_jac_block4=digest(Xj.cpu().numpy()))
    print("RESULT " + json.dumps(dict(ms=t, bits=bits)), flush=True)
    for d in (dv, dc, dj):
        d.close()


def regress(other_lib, out_path):
    res, bits = {"this": {}, "other": {}}, {}
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
            print(f"round {rnd + 1}, {which}: done", flush=True)
    out = {w: {k: stat(v) for k, v in d.items()} for w, d in res.items()}
    out["same_bits"] = {k: bits["this"][k] == bits["other"][k] for k in bits["this"]}
    for k in res["this"]:
        print(f"{k}: this {fmt(out['this'][k])} ms   other {fmt(out['other'][k])} ms   same bits: {out['same_bits'][k]}", flush=True)
    if out_path:
        json.dump(out, open(out_path, "w"), indent=1)


def rehearse():
    import multigrid_jl_amd as mg
    import vanka_cases as V
    for omega in (OMEGA, None):
        A = V.mixed_operator([8] * 3, True, omega=omega)
        print("byte model at 8^3:", byte_model(mg, A, [8] * 3), "per cell", sum(byte_model(mg, A, [8] * 3)) / 512)
    p = mg.getMGparam(np.complex128, np.int64, 4, 1, 1, 1e-8, "VankaFaces", 0.6, 1, 1, "V", "NoMUMPS", 0.4, 0.0, MIXED, complexVanka=True)
    mg.MGsetup(V.mixed_operator([16] * 3, True, omega=OMEGA), mg.getRegularMesh([0, 1] * 3, [16] * 3), p)
    print("levels", p.levels, [M.shape[0] for M in p.As])


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "rehearse"
    if mode == "rehearse":
        rehearse()
    elif mode == "child":
        child()
    elif mode == "build":
        build(int(sys.argv[2]), sys.argv[3] if len(sys.argv) > 3 else None)
    elif mode == "resetup":
        resetup(sys.argv[2] if len(sys.argv) > 2 else None)
    elif mode == "regress":
        regress(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        sys.exit(f"unknown mode {mode}")
