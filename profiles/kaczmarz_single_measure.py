"""Measurements behind profiles/kaczmarz_single.md (Float32 / ComplexF32 hybrid Kaczmarz on the device).
    python profiles/kaczmarz_single_measure.py [--parent-lib LIB.so] [--out FILE.json] [--cells2 N --cells3 N]
Time per sweep of the PARALLEL schedule (one wavefront per sub-domain) through mg_kaczmarz_apply_dev_* on device-resident
x and b: a 2-D Helmholtz operator of 512^2 cells with 16 x 16 sub-domains and a 3-D one of 64^3 cells with 4 x 4 x 4
sub-domains, 1 and 4 columns, FP32 against FP64 (the real part of the operator) and CFP32 against CFP64, in one process:
ROUNDS alternating rounds, each one call of SWEEPS sweeps behind a warm-up call, host clock around the call (it ends in
a synchronise of the library's stream); medians with min - max.  Each timed call starts from x = 0.
--parent-lib: the parent commit's libmgvcycle.so; its mg_kaczmarz_*_CFP64 entry points are timed in the same rounds on the
same operators, and a SHA-256 of the SEQUENTIAL schedule's result (the parallel one races) is compared with this tree's."""
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
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--cells2", type=int, default=512)
ap.add_argument("--cells3", type=int, default=64)
args = ap.parse_args()
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.join(HERE, "tests"))
import multigrid_jl_amd as mg   # noqa: E402
from multigrid_jl_amd import par_relax   # noqa: E402
from complex_cases import helmholtz   # noqa: E402

D = mg.device
lib = D.load_library()
ROUNDS, SWEEPS = 5, 20
KINDS = {"FP64": (np.float64, False), "CFP64": (np.complex128, False), "FP32": (np.float32, True), "CFP32": (np.complex64, True)}
TORCH = {"FP64": torch.float64, "CFP64": torch.complex128, "FP32": torch.float32, "CFP32": torch.complex64}


def stats(v):
    v = np.asarray(v, dtype=float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def parent_entry_points(path):
    """The parent library's CFP64 entry points (another copy of the library in this process)."""
    P = C.CDLL(path)
    ll, vp, dp, lp = C.c_longlong, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong)
    P.mg_kaczmarz_create_CFP64_INT64.argtypes = [ll, ll, lp, dp, lp, ll, ll, C.POINTER(C.c_uint), dp, C.POINTER(vp)]
    P.mg_kaczmarz_apply_dev_CFP64.argtypes = [vp, vp, vp, ll, ll, ll]
    P.mg_kaczmarz_destroy.argtypes = [vp]
    return P


def parent_handle(P, A, hk):
    cp = np.ascontiguousarray(A.indptr, dtype=np.int64) + 1
    rv = np.ascontiguousarray(A.indices, dtype=np.int64) + 1
    nz = np.ascontiguousarray(np.conj(A.data), dtype=np.complex128)
    arr = np.asfortranarray(hk.ArrIdxs, dtype=np.uint32)
    inv = np.ascontiguousarray(hk.invDiag, dtype=np.complex128)
    h = C.c_void_p()
    rc = P.mg_kaczmarz_create_CFP64_INT64(0, A.shape[0], D._i64(cp), D._f64(nz), D._i64(rv), arr.shape[1], arr.shape[0],
                                          arr.ctypes.data_as(C.POINTER(C.c_uint)), D._f64(inv), C.byref(h))
    assert rc == 0
    return h


def timed(fn, h, x, b, nrhs):
    x.zero_()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = fn(h, x.data_ptr(), b.data_ptr(), nrhs, SWEEPS, 0)
    dt = time.perf_counter() - t0
    assert rc == 0 and bool(torch.isfinite(torch.view_as_real(x) if x.is_complex() else x).all())
    return dt * 1e3 / SWEEPS


def operator(name, cells, domains):
    A, mesh = helmholtz(mg, cells)
    A = A.tocsr()
    A.sort_indices()
    out = dict(name=name, cells=cells, domains=domains, n=int(A.shape[0]), nnz=int(A.nnz), rows=[])
    H, M = {}, {}
    for kind, (VAL, single) in KINDS.items():
        Ak = (A if np.dtype(VAL).kind == "c" else A.real).astype(VAL).tocsr()
        kw = dict(singleValues=True) if single else {}
        hk = mg.getHybridKaczmarz(VAL, np.int64, Ak, mesh, domains, mg.getNodalIndicesOfCell, 0.8, 4, SWEEPS, **kw)
        H[kind], M[kind] = hk, Ak
        par_relax._device_handle(hk, Ak)
    out["domain_length"] = int(H["FP64"].ArrIdxs.shape[0])
    P = parent_entry_points(args.parent_lib) if args.parent_lib else None
    hp = parent_handle(P, M["CFP64"], H["CFP64"]) if P else None
    n = A.shape[0]
    for nrhs in (1, 4):
        rng = np.random.default_rng(5 + nrhs)
        b64 = rng.standard_normal((nrhs, n)) + 1j * rng.standard_normal((nrhs, n))
        b64 /= np.linalg.norm(b64)
        B = {k: torch.from_numpy(np.ascontiguousarray((b64 if KINDS[k][0] in (np.complex128, np.complex64) else b64.real)
                                                      .astype(KINDS[k][0]))).cuda() for k in KINDS}
        X = {k: torch.zeros_like(B[k]) for k in KINDS}
        fns = {k: (getattr(lib, f"mg_kaczmarz_apply_dev_{k}"), H[k]._handle, X[k], B[k]) for k in KINDS}
        if P:
            fns["CFP64_parent"] = (P.mg_kaczmarz_apply_dev_CFP64, hp, torch.zeros_like(B["CFP64"]), B["CFP64"])
        for f, h, x, b in fns.values():            # warm-up: code objects, first touch
            timed(f, h, x, b, nrhs)
        samples = {k: [] for k in fns}
        for r in range(ROUNDS):
            order = list(fns) if r % 2 == 0 else list(fns)[::-1]
            for k in order:
                f, h, x, b = fns[k]
                samples[k].append(timed(f, h, x, b, nrhs))
        row = dict(nrhs=nrhs, ms_per_sweep={k: stats(v) for k, v in samples.items()})
        med = {k: row["ms_per_sweep"][k]["median"] for k in samples}
        row["FP64_over_FP32"] = med["FP64"] / med["FP32"]
        row["CFP64_over_CFP32"] = med["CFP64"] / med["CFP32"]
        # what the sweeps did: relative residual after SWEEPS parallel sweeps from x = 0 (computed in double on the host)
        res = {}
        for k in KINDS:
            xk = X[k].cpu().numpy().astype(np.complex128).T
            bk = B[k].cpu().numpy().astype(np.complex128).T
            res[k] = float(np.linalg.norm(M[k].astype(np.complex128) @ xk - bk) / np.linalg.norm(bk))
        row["relres_after_sweeps"] = res
        if P:
            row["CFP64_parent_over_this"] = med["CFP64_parent"] / med["CFP64"]
            # the same bits: the sequential schedule (deterministic), 2 sweeps
            xa, xb = torch.zeros_like(B["CFP64"]), torch.zeros_like(B["CFP64"])
            assert lib.mg_kaczmarz_apply_dev_CFP64(H["CFP64"]._handle, xa.data_ptr(), B["CFP64"].data_ptr(), nrhs, 2, 1) == 0
            assert P.mg_kaczmarz_apply_dev_CFP64(hp, xb.data_ptr(), B["CFP64"].data_ptr(), nrhs, 2, 1) == 0
            row["CFP64_sequential_sha"] = dict(this=sha(xa.cpu().numpy()), parent=sha(xb.cpu().numpy()))
            assert row["CFP64_sequential_sha"]["this"] == row["CFP64_sequential_sha"]["parent"]
        print(name, json.dumps(row), flush=True)
        out["rows"].append(row)
    for hk in H.values():
        hk.close()
    if P:
        P.mg_kaczmarz_destroy(hp)
    return out


res = dict(rounds=ROUNDS, sweeps_per_call=SWEEPS, parent_lib=bool(args.parent_lib),
           operators=[operator("helmholtz2d", [args.cells2] * 2, [16, 16]), operator("helmholtz3d", [args.cells3] * 3, [4, 4, 4])])
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)
