"""-m gpu: what the complex entry points refuse, vector form beside block form, on the MI355X.

Every vector entry point of the complex path has a block twin (mg_cycle_CF64 / mg_block_cycle_CF64, mg_bicgstab_CFP64 /
mg_block_bicgstab_CFP64, ...).  Both forms go through the same checks, and a call with ONE invalid argument gets the return code and
the mg_last_error text of its own form: "null vector" against "null block", "... for device vectors" against "... for device
blocks".  TABLE holds one row per entry point and invalid argument: (entry point, fault, handle, code, text).  Every row is refused
on the host before anything is launched; afterwards the handle still cycles a vector and a block of three columns to the bounds of
tests/test_complex_block_gpu.py (1e-12 against the complex oracle)."""
import ctypes as C

import numpy as np
import pytest
import torch

import complex_block_oracle as cb
import complex_oracle as corc
from complex_cases import complex_rhs, helmholtz

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 4
KMAX = 16

# ---- the entry points: (vector | block, host | device pointers, the arguments between n and the outputs) ----------------------------
HOST_VEC = ["mg_cycle_CF64", "mg_solve_CF64", "mg_spmv_CF64"]
HOST_VEC32 = ["mg_cycle_CF32", "mg_solve_CF32", "mg_spmv_CF32"]
HOST_BLK = ["mg_block_cycle_CF64", "mg_block_solve_CF64", "mg_block_spmv_CF64"]
KRY_VEC = ["mg_bicgstab_CFP64", "mg_bicgstab_dev_CFP64", "mg_fgmres_CFP64", "mg_fgmres_dev_CFP64"]
KRY_BLK = ["mg_block_bicgstab_CFP64", "mg_block_bicgstab_dev_CFP64", "mg_block_fgmres_CFP64", "mg_block_fgmres_dev_CFP64"]
DEV_VEC, DEV_BLK = "mg_cycle_dev_CFP64", "mg_block_cycle_dev_CFP64"
CG_VEC, CG_BLK = "mg_coarse_gmres_CF64", "mg_block_coarse_gmres_CF64"
ANY_VEC = KRY_VEC + [DEV_VEC]            # the _CFP64 entry points serve CF64 and CF32 handles
ANY_BLK = KRY_BLK + [DEV_BLK]
ALL_BLK = HOST_BLK + ANY_BLK

# ---- the refusals, as the library words them --------------------------------------------------------------------------------------
NULL_VEC, NULL_BLK, NULL_ARG = "null vector", "null block", "null argument"
FINE_N = "does not match the fine level"
COARSE_N = "does not match the coarsest level"
ONE_RHS = "complex handles serve one right-hand side (nrhs=2)"
NRHS_LOW = "nrhs=0: a block holds at least one right-hand side"
NRHS_HIGH = "complex blocks hold at most 16 right-hand sides (nrhs=17)"
XZ_VEC = "x_is_zero must be 0 or 1 for device vectors"
XZ_BLK = "x_is_zero must be 0 or 1 for device blocks"
MAXIT = "maxIter < 0"
INNER = "inner must be in [1,64]"
KCYCLE = "blocks of right-hand sides are not served on a K-cycle / Jac-GMRES complex hierarchy"
GMRES = "blocks of right-hand sides are not served on a complex hierarchy with the GMRES coarsest solve (nrhs=2)"


def _null(e, vec):
    return NULL_ARG if "spmv" in e else (NULL_VEC if vec else NULL_BLK)


# handles: c64 / c32 - Helmholtz 8^3, two levels, Jac V(1,1), ComplexF64 / ComplexF32; kc - the same with the K-cycle;
# gm - the same with the GMRES coarsest solve, blocks on it not asked for
TABLE = []
for hd, vec_host in (("c64", HOST_VEC), ("c32", HOST_VEC32)):
    for e in vec_host + ANY_VEC:
        TABLE += [(e, {"b": None}, hd, INVALID, _null(e, True)), (e, {"x": None}, hd, INVALID, _null(e, True))]
        if "spmv" not in e:
            TABLE.append((e, {"dn": 1}, hd, INVALID, FINE_N))
    TABLE += [(e, {"nrhs": 2}, hd, UNSUPPORTED, ONE_RHS) for e in vec_host]
    TABLE.append((DEV_VEC, {"xz": 2}, hd, INVALID, XZ_VEC))
    TABLE += [(e, {"maxIter": -1}, hd, INVALID, MAXIT) for e in [vec_host[1]] + KRY_VEC]
    TABLE += [(e, {"inner": i}, hd, INVALID, INNER) for e in KRY_VEC[2:] + KRY_BLK[2:] for i in (0, 65)]
    for e in (HOST_BLK if hd == "c64" else []) + ANY_BLK:
        TABLE += [(e, {"b": None}, hd, INVALID, _null(e, False)), (e, {"x": None}, hd, INVALID, _null(e, False)),
                  (e, {"nrhs": 0}, hd, INVALID, NRHS_LOW), (e, {"nrhs": 17}, hd, UNSUPPORTED, NRHS_HIGH)]
        if "spmv" not in e:
            TABLE.append((e, {"dn": 1}, hd, INVALID, FINE_N))
    TABLE.append((DEV_BLK, {"xz": 2}, hd, INVALID, XZ_BLK))
    TABLE += [(e, {"maxIter": -1}, hd, INVALID, MAXIT) for e in ([HOST_BLK[1]] if hd == "c64" else []) + KRY_BLK]
TABLE += [(e, {}, "kc", UNSUPPORTED, KCYCLE) for e in ALL_BLK]
TABLE += [(e, {}, "gm", UNSUPPORTED, GMRES) for e in ALL_BLK + [CG_BLK]]
TABLE += [(CG_VEC, {"b": None}, "gm", INVALID, NULL_VEC), (CG_VEC, {"x": None}, "gm", INVALID, NULL_VEC),
          (CG_VEC, {"dn": 1}, "gm", INVALID, COARSE_N),
          (CG_BLK, {"b": None, "nrhs": 1}, "gm", INVALID, NULL_BLK), (CG_BLK, {"x": None, "nrhs": 1}, "gm", INVALID, NULL_BLK),
          (CG_BLK, {"dn": 1, "nrhs": 1}, "gm", INVALID, COARSE_N),
          (CG_BLK, {"nrhs": 0}, "gm", INVALID, NRHS_LOW), (CG_BLK, {"nrhs": 17}, "gm", UNSUPPORTED, NRHS_HIGH)]


def _param(mg, A, mesh, cyc="V", coarse="NoMUMPS", single=False):
    kw = {"singlePrecision": True} if single else {}
    p = mg.getMGparam(np.complex128, np.int64, 2, 8, 4, 1e-10, "Jac", 0.8, 1, 1, cyc, coarse, 0.5, 0.0, **kw)
    mg.MGsetup(A, mesh, p)
    return p


def _columns_close(X, Xo, tol):
    for j in range(X.shape[1]):
        scale = np.abs(Xo[:, j]).max()
        assert np.abs(X[:, j] - Xo[:, j]).max() <= tol * scale, (j, np.abs(X[:, j] - Xo[:, j]).max() / scale)


def test_single_faults_are_refused_in_the_words_of_their_form(mg, built):
    lib = mg.device.load_library()
    A, mesh = helmholtz(mg, [8, 8, 8], 0.5, 0.5)
    n = A.shape[0]
    params = {"c64": _param(mg, A, mesh), "c32": _param(mg, A, mesh, single=True), "kc": _param(mg, A, mesh, cyc="K"),
              "gm": _param(mg, A, mesh, coarse="GMRES")}
    devs = {}
    try:
        for key, p in params.items():
            devs[key] = mg.device.DeviceHierarchy(p)
        n_coarse = params["gm"].As[-1].shape[0]
        host = {8: np.zeros(2 * n * (KMAX + 1)), 4: np.zeros(2 * n * (KMAX + 1), dtype=np.float32)}
        host_x = {w: a.copy() for w, a in host.items()}
        ab = {8: np.array([1.0, 0.0]), 4: np.array([1.0, 0.0], dtype=np.float32)}
        res = np.zeros(512)
        bd = torch.zeros((n, KMAX + 1), dtype=torch.complex128, device="cuda")
        xd = torch.zeros_like(bd)
        torch.cuda.synchronize()
        out = [C.c_longlong(0) for _ in range(3)]
        lp = [C.byref(o) for o in out]
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))

        def call(entry, fault, hd):
            a = dict(b=1, x=1, dn=0, nrhs=2 if "block" in entry else 1, xz=1, maxIter=2, inner=3)
            a.update(fault)
            if "_dev_" in entry:
                b, x = C.c_void_p(bd.data_ptr()), C.c_void_p(xd.data_ptr())
            else:
                w, ptr = (4, fp) if entry.endswith("CF32") else (8, dp)
                b, x = ptr(host[w]), ptr(host_x[w])
            b, x = (None if a["b"] is None else b), (None if a["x"] is None else x)
            nn = (n_coarse if "coarse_gmres" in entry else n) + a["dn"]
            cols = (a["nrhs"],) if "block" in entry else ()
            stem = entry[3:].rsplit("_", 1)[0].replace("block_", "")
            if stem == "cycle":
                args = (b, x, nn, a["nrhs"], a["xz"])
            elif stem == "solve":
                args = (b, x, nn, a["nrhs"], 1e-6, a["maxIter"], lp[0], dp(res))
            elif stem == "spmv":
                al = (fp if entry.endswith("CF32") else dp)(ab[4 if entry.endswith("CF32") else 8])
                args = (1, mg.device.MG_OP_A, al, b, al, x, a["nrhs"])
            elif stem == "cycle_dev":
                args = (b, x, nn) + cols + (a["xz"],)
            elif stem in ("bicgstab", "bicgstab_dev"):
                args = (b, x, nn) + cols + (1e-6, a["maxIter"], lp[0], lp[1], dp(res), lp[2])
            elif stem in ("fgmres", "fgmres_dev"):
                args = (b, x, nn) + cols + (a["inner"], 1e-6, a["maxIter"], lp[0], lp[1], dp(res), lp[2])
            else:
                assert stem == "coarse_gmres", entry
                args = (b, x, nn) + cols + (lp[0], lp[1], dp(res))
            rc = getattr(lib, entry)(devs[hd].handle, *args)
            msg = lib.mg_last_error()
            return rc, (msg.decode() if msg else "")

        wrong = []
        for entry, fault, hd, code, text in TABLE:
            rc, msg = call(entry, fault, hd)
            if rc != code or text not in msg:
                wrong.append((entry, fault, hd, code, text, rc, msg))
        print(f"  {len(TABLE)} rows, {len(wrong)} wrong")
        for w in wrong:
            print("  WRONG", w)
        assert not wrong
        torch.cuda.synchronize()
        assert not bd.any() and not xd.any() and not any(a.any() for a in host_x.values())     # nothing ran
        # the handle the refusals went to still serves both forms
        dev, p = devs["c64"], params["c64"]
        b = complex_rhs(n, 15)
        x = np.zeros_like(b)
        dev.cycle(b, x, 1)
        xo = corc.recursiveCycle(p, b, np.zeros_like(b), 1)
        assert np.abs(x - xo).max() <= 1e-12 * np.abs(xo).max()
        B = np.asfortranarray(np.stack([complex_rhs(n, 80 + j) for j in range(3)], axis=1))
        X = np.zeros((n, 3), dtype=np.complex128, order="F")
        dev.block_cycle(B, X, 1)
        _columns_close(X, cb.block_cycle(p, B, np.zeros((n, 3), dtype=np.complex128)), 1e-12)
    finally:
        for d in devs.values():
            d.close()
        for p in params.values():
            mg.clear_(p)
