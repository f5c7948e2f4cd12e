"""MG-preconditioned PCG / BiCGSTAB / FGMRES on the HALO form of the sharded hierarchy (general CSR: SA-AMG) against the oracle's
solveCG_MG / solveBiCGSTAB_MG / solveGMRES_MG on the same host-built hierarchy.

CPU (-m "not gpu"): the Python sequencer (DistributedHierarchy.pcg / bicgstab / fgmres) under gloo with the checker backend.
GPU (-m gpu): mg_dist_pcg_dev_FP64 / mg_dist_bicgstab_dev_FP64 / mg_dist_fgmres_dev_FP64 through NativeDistributedHierarchy - two
processes sharing the GPU over the plug-in transport, a world of one over RCCL - and the fused vector passes (csrc/mg_krvec.hpp)
on their own against numpy in long double.

Everywhere: flag and count equal on every rank, every rank's resvec within 1e-10 * max(1, max|resvec_ref|) of the oracle's and of
the same length, the gathered x within 1e-10 * max|x_ref| (the tolerances of the ghost-layer form's drivers); tol = 1e-9,
maxIter = 40 ("sa") / 12 ("gmg3d"), FGMRES(3), BiCGSTAB from a seeded non-zero x0.  The communication outside the preconditioner is
asserted as counts: one level-1 exchange per product with A; all-reduces per iteration at most 2 (PCG), 3 (BiCGSTAB), 2 per inner
step (FGMRES)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dist_krylov_helpers as hk  # noqa: E402


# ---- CPU: the Python sequencer under gloo ----------------------------------------------------------------------------------
@pytest.mark.parametrize("world,kind,cyc,method", [(2, "sa", "V", "pcg"), (4, "sa", "V", "pcg"), (2, "sa", "V", "bicgstab"),
                                                   (4, "sa", "V", "bicgstab"), (2, "gmg3d", "V", "fgmres"), (4, "gmg3d", "V", "fgmres"),
                                                   (2, "gmg3d", "W", "pcg")])
def test_halo_form_krylov_cpu_vs_oracle(built, world, kind, cyc, method):
    k, infos = hk.run(world, kind, cyc, method, "cpu")
    hk.check_communication(method, k, infos)


def test_python_sequencer_refuses_blocks(built):
    from multigrid_jl_amd import distributed as dd
    H = dd.DistributedHierarchy.__new__(dd.DistributedHierarchy)
    H.nrhs, H.relaxType, H.cycleType, H._kry = 2, "Jac", "V", None
    with pytest.raises(NotImplementedError):
        H.pcg(None, None, 1e-9, 1)


def test_library_exports_the_halo_form_drivers(mg, built):
    """Fails without the feature: the parent's library has none of these symbols."""
    lib = ctypes.CDLL(mg.device.LIB_PATH)
    for name in ("mg_dist_pcg_dev_FP64", "mg_dist_bicgstab_dev_FP64", "mg_dist_fgmres_dev_FP64", "mg_dist_stats", "mg_vec_dots_dev_FP64",
                 "mg_vec_pcg_update_dev_FP64", "mg_vec_bicg_xr_dev_FP64", "mg_vec_gs_update_dev_FP64"):
        assert hasattr(lib, name), name
        assert name in mg.device.SIGNATURES


# ---- GPU: the native sequencer -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("world,kind,cyc,method,mode,box", [(2, "sa", "V", "pcg", "plugin", False), (2, "sa", "V", "bicgstab", "plugin", False),
                                                           (2, "gmg3d", "V", "fgmres", "plugin", True), (1, "sa", "V", "pcg", "rccl", False)])
def test_halo_form_krylov_hip_vs_oracle(built, world, kind, cyc, method, mode, box):
    k, infos = hk.run(world, kind, cyc, method, mode, box=box)
    if world > 1:
        hk.check_communication(method, k, infos)


# ---- GPU: the fused passes alone ----------------------------------------------------------------------------------------------
from krylov_bounds import LD, _close_sum, _close_vec, _ld  # noqa: E402  (shared with the real drivers' kernel-level test)


def _vectors(n, count, layout, seed):
    """`count` seeded device vectors of n doubles.  layout 0: on a 16-byte boundary; 1: 8 bytes past one; 2: mixed (every other one)."""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(count):
        base = torch.zeros(n + 2, dtype=torch.float64, device="cuda")
        assert base.data_ptr() % 16 == 0
        off = 1 if (layout == 1 or (layout == 2 and c % 2 == 1)) else 0
        v = base[off: off + n]
        v.copy_(torch.from_numpy(rng.standard_normal(n)))
        assert v.data_ptr() % 16 == 8 * off
        out.append(v)
    return out


def _passes(D, n, layout):
    """Every fused pass once on fresh seeded vectors; returns {name: (tensors written, sums)} after checking them."""
    ws = torch.zeros(D.KRV_WORKSPACE, dtype=torch.float64, device="cuda")
    out = torch.zeros(8, dtype=torch.float64, device="cuda")
    alpha, beta, omega = 0.37, -1.3, 0.81
    res = {}

    def sums(k):
        torch.cuda.synchronize()
        return out[:k].cpu().numpy().copy()

    a, b, c = _vectors(n, 3, layout, 1)
    D.vec_dots([a, a, c], [b, a, b], n, ws, out)
    s = sums(3)
    for j, (x, y) in enumerate(((a, b), (a, a), (c, b))):
        _close_sum(f"dots[{j}]", s[j], _ld(x) * _ld(y))
    res["dots"] = ([], s)

    p, q, r = _vectors(n, 3, layout, 2)
    D.vec_pcg_dots(p, q, r, n, ws, out)
    s = sums(3)
    _close_sum("pcg_dots p'q", s[0], _ld(p) * _ld(q))
    _close_sum("pcg_dots r'q", s[1], _ld(r) * _ld(q))
    _close_sum("pcg_dots q'q", s[2], _ld(q) * _ld(q))
    res["pcg_dots"] = ([], s)

    p, q, x, r = _vectors(n, 4, layout, 3)
    x0, r0 = _ld(x), _ld(r)
    D.vec_pcg_update(alpha, p, q, x, r, n, ws, out)
    s = sums(1)
    _close_vec("pcg_update x", x, x0 + LD(alpha) * _ld(p), x0, LD(alpha) * _ld(p))
    _close_vec("pcg_update r", r, r0 - LD(alpha) * _ld(q), r0, LD(alpha) * _ld(q))
    _close_sum("pcg_update r'r", s[0], _ld(r) * _ld(r))
    res["pcg_update"] = ([x.clone(), r.clone()], s)

    x, y = _vectors(n, 2, layout, 4)
    y0 = _ld(y)
    D.vec_xpby(x, beta, y, n)
    torch.cuda.synchronize()
    _close_vec("xpby", y, _ld(x) + LD(beta) * y0, _ld(x), LD(beta) * y0)
    res["xpby"] = ([y.clone()], np.zeros(0))

    x, y = _vectors(n, 2, layout, 5)
    D.vec_scale(alpha, x, y, n)
    torch.cuda.synchronize()
    _close_vec("scale", y, LD(alpha) * _ld(x))
    res["scale"] = ([y.clone()], np.zeros(0))

    r, v, p = _vectors(n, 3, layout, 6)
    p0 = _ld(p)
    D.vec_bicg_p(beta, omega, r, v, p, n)
    torch.cuda.synchronize()
    inner = p0 - LD(omega) * _ld(v)
    _close_vec("bicg_p", p, _ld(r) + LD(beta) * inner, _ld(r), p0, LD(omega) * _ld(v), inner, LD(beta) * inner)
    res["bicg_p"] = ([p.clone()], np.zeros(0))

    v, r = _vectors(n, 2, layout, 7)
    r0 = _ld(r)
    D.vec_bicg_s(alpha, v, r, n, ws, out)
    s = sums(1)
    _close_vec("bicg_s", r, r0 - LD(alpha) * _ld(v), r0, LD(alpha) * _ld(v))
    _close_sum("bicg_s s's", s[0], _ld(r) * _ld(r))
    res["bicg_s"] = ([r.clone()], s)

    t, sv = _vectors(n, 2, layout, 8)
    D.vec_bicg_ts(t, sv, n, ws, out)
    s = sums(2)
    _close_sum("bicg_ts t's", s[0], _ld(t) * _ld(sv))
    _close_sum("bicg_ts t't", s[1], _ld(t) * _ld(t))
    res["bicg_ts"] = ([], s)

    phat, shat, t, rtld, x, r = _vectors(n, 6, layout, 9)
    x0, r0 = _ld(x), _ld(r)
    D.vec_bicg_xr(alpha, omega, phat, shat, t, rtld, x, r, n, ws, out)
    s = sums(2)
    upd = LD(alpha) * _ld(phat) + LD(omega) * _ld(shat)
    _close_vec("bicg_xr x", x, x0 + upd, x0, LD(alpha) * _ld(phat), LD(omega) * _ld(shat), upd)
    _close_vec("bicg_xr r", r, r0 - LD(omega) * _ld(t), r0, LD(omega) * _ld(t))
    _close_sum("bicg_xr r'r", s[0], _ld(r) * _ld(r))
    _close_sum("bicg_xr rtld'r", s[1], _ld(rtld) * _ld(r))
    res["bicg_xr"] = ([x.clone(), r.clone()], s)

    for m in (3, 10):        # one pass / two passes of 8 vectors at most; the reference: one rounded update after the other
        vs = _vectors(n, m + 1, layout, 10 + m)
        w, vs = vs[0], vs[1:]
        h = np.random.default_rng(20 + m).standard_normal(m)
        ref, mag = _ld(w), np.abs(_ld(w))
        for hj, v in zip(h, vs):
            term = LD(hj) * _ld(v)
            mag = np.maximum(mag, np.maximum(np.abs(term), np.abs(ref)))
            ref = (ref - term).astype(np.float64).astype(LD)
        D.vec_gs_update(h, vs, w, n, ws, out)
        s = sums(1)
        _close_vec(f"gs_update m={m}", w, ref, mag)
        _close_sum(f"gs_update m={m} w'w", s[0], _ld(w) * _ld(w))
        res[f"gs_update{m}"] = ([w.clone()], s)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1_000_003])
@pytest.mark.parametrize("layout", [0, 1, 2])
def test_fused_passes_vs_long_double(mg, built, n, layout):
    """Updated vectors within 2 ulp of the unfused expression, every sum within n * 2^-53 * sum|terms| of the long-double sum, two runs
    bit-identical; vectors on a 16-byte boundary, 8 bytes past one (the 16-byte path behind one scalar element), and mixed."""
    D = mg.device
    D.load_library()
    print(f"  n = {n}, layout {layout}")
    first = _passes(D, n, layout)
    second = _passes(D, n, layout)
    for name, (tensors, s) in first.items():
        t2, s2 = second[name]
        assert np.array_equal(s, s2), (name, s, s2)                       # bit-identical sums ...
        for u, v in zip(tensors, t2):
            assert torch.equal(u, v), name                                # ... and vectors
