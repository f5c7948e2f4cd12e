"""Device time of the complex triangular solve (profiles/parlu_complex.md): 256 x 256 Helmholtz factor, 1 and 16 right-hand
sides, plain and adjoint: (a) chip-wide complex, (b) single-workgroup complex, (c) real applier on a real matrix of the same
pattern; then (a) against (b) on smaller factors for the crossover.  mg_lu_time_dev: 3 warm-up solves, median of the repeats,
events on the library's stream, device vectors.  Run on the GPU from the repository root after the build:
    python profiles/parlu_complex_measure.py [out.json]"""
import ctypes as C, json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # profiles/ -> repository root
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import scipy.sparse as sp
import multigrid_jl_amd as mg
from complex_cases import helmholtz, lu_layout
from parlu_complex_cases import factor

lib = mg.device.load_library()
I, F = mg.device._i64, mg.device._f64
A, _ = helmholtz(mg, [256, 256])
A = A.tocsc()
n = A.shape[0]
t0 = time.time(); luc = factor(A); print("complex splu", time.time() - t0, flush=True)
# a definite real matrix of the same pattern: Laplacian + shift
Ar = (A.real + 2.0 * (0.5 * 0.5) * (A.real.diagonal().max() / 4.0) * sp.identity(n)).tocsc()
t0 = time.time(); lur = factor(Ar); print("real splu", time.time() - t0, flush=True)
Fc, Fr = lu_layout(luc), lu_layout(lur)
Fr["Lv"], Fr["Uv"] = np.ascontiguousarray(Fr["Lv"].real), np.ascontiguousarray(Fr["Uv"].real)
args = lambda G: (0, n, I(G["Lp"]), I(G["Lc"]), F(G["Lv"]), I(G["Up"]), I(G["Uc"]), F(G["Uv"]), I(G["p"]), I(G["q"]))
out = {"n": n, "nnzL_complex": int(Fc["Lp"][-1] - 1), "nnzU_complex": int(Fc["Up"][-1] - 1), "nnzL_real": int(Fr["Lp"][-1] - 1),
       "nnzU_real": int(Fr["Up"][-1] - 1), "rows": []}

def handle(create, G, env):
    for k, v in env.items(): os.environ[k] = v
    h = C.c_void_p()
    rc = create(*args(G), C.byref(h))
    for k in env: del os.environ[k]
    assert rc == 0, lib.mg_last_error()
    return h

def form(h, t):
    info = np.zeros(7, dtype=np.int64)
    assert lib.mg_lu_form(h, t, I(info)) == 0
    return [int(v) for v in info]

def timed(h, cplx, nrhs, t, reps):
    w = 2 if cplx else 1
    b = torch.randn(n, nrhs * w, dtype=torch.float64, device="cuda")
    x = torch.zeros_like(b)
    torch.cuda.synchronize()
    ms = np.zeros(reps)
    rc = lib.mg_lu_time_dev(h, b.data_ptr(), x.data_ptr(), n, nrhs, t, 3, reps, F(ms))
    assert rc == 0, lib.mg_last_error()
    assert bool(torch.isfinite(x).all())
    return float(np.median(ms)), float(ms.min()), float(ms.max())

forms = (("a_chipwide_complex", lib.mg_lu_create_CFP64_INT64, Fc, {}, True, 30),
         ("c_real_chipwide", lib.mg_lu_create_FP64_INT64, Fr, {}, False, 30),
         ("b_single_wg_complex", lib.mg_lu_create_CFP64_INT64, Fc, {"MG_LU_MULTI_MIN_ROWS": "1000000000"}, True, 5))
for name, create, G, env, cplx, reps in forms:
    h = handle(create, G, env)
    for t in (0, 1):
        f = form(h, t)
        for nrhs in (1, 16):
            med, lo, hi = timed(h, cplx, nrhs, t, reps)
            row = dict(form=name, doTranspose=t, nrhs=nrhs, median_ms=med, min_ms=lo, max_ms=hi, info=f)
            print(json.dumps(row), flush=True)
            out["rows"].append(row)
    lib.mg_lu_destroy(h)
# crossover: smaller Helmholtz factors, chip-wide against single workgroup, nrhs 1, plain
for cells in (32, 64, 128):
    A2, _ = helmholtz(mg, [cells, cells]); A2 = A2.tocsc(); n = A2.shape[0]
    G = lu_layout(factor(A2))
    for name, env in (("a_chipwide_complex", {"MG_LU_MULTI_MIN_ROWS": "0"}), ("b_single_wg_complex", {"MG_LU_MULTI_MIN_ROWS": "1000000000"})):
        h = handle(lib.mg_lu_create_CFP64_INT64, G, env)
        f = form(h, 0)
        for nrhs in (1, 16):
            med, lo, hi = timed(h, True, nrhs, 0, 10)
            row = dict(form=name, cells=cells, n=n, doTranspose=0, nrhs=nrhs, median_ms=med, min_ms=lo, max_ms=hi, info=f)
            print(json.dumps(row), flush=True)
            out["rows"].append(row)
        lib.mg_lu_destroy(h)
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
