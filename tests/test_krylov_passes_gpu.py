"""The passes of the real single-GPU Krylov drivers (pcg_dev, bicgstab_dev, FgmresCore, the block drivers: csrc/mg_krylov.inc) one by one
on the device, through mg_kry_*_dev_FP64 - the helpers the drivers themselves call - and mg_vec_dscale / xpdr / sumsq_dev_FP64, against
numpy long double (tests/krylov_pass_cases.py: shapes, bounds and their derivation; tests/test_krylov_passes_host.py: the bounds hold for
a plain restatement and reject wrong variants).  Every output lives between guard zones of a signalling-NaN bit pattern, every input is
compared bit for bit after the call, every pass runs twice and must give the same bits (no atomics in this family).  Vectors sit on a
16-byte boundary, 8 bytes past one (what the drivers pass to the pair kernels whenever n is odd: BiCGSTAB's t = kw + n, FGMRES's
V + k n, the Jacobi-GMRES coarsest solve on 5^3 or 9^3 rows) and mixed.  n is the caller's: one small two-level handle serves all."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import krylov_pass_cases as kc  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = kc.GUARD


@pytest.fixture(scope="module")
def dev(mg, built):
    A, mesh = mg.poisson_shifted([8, 8])
    p = mg.getMGparam(np.float64, np.int64, 2, 8, 4, 1e-10, "Jac", 0.8, 1, 1, "V")
    mg.MGsetup(A, mesh, p)
    d = mg.device.DeviceHierarchy(p)
    yield d
    d.close()


class Guarded:
    """`data` (any shape, float64) as a contiguous device view `off` doubles past a 16-byte boundary, between guard zones of SENTINEL
    (`tail` more doubles of it behind the view)."""

    def __init__(self, data, off=0, tail=0):
        self.data = np.ascontiguousarray(data, dtype=np.float64).copy()
        size = self.data.size
        self.lo = GUARD + off
        self.base = torch.empty(size + 2 * GUARD + 2 + tail, dtype=torch.float64, device="cuda")
        self.base.view(torch.int64).fill_(int(kc.SENTINEL))
        assert self.base.data_ptr() % 16 == 0
        self.v = self.base[self.lo:self.lo + size].view(self.data.shape)
        self.v.copy_(torch.from_numpy(self.data))
        assert self.v.is_contiguous() and self.v.data_ptr() % 16 == 8 * off

    def host(self):
        """The view on the host after checking both guard zones bit for bit."""
        torch.cuda.synchronize()
        base = self.base.cpu().numpy()
        hi = self.lo + self.data.size
        ok = np.all(base[:self.lo].view(np.int64) == kc.SENTINEL) and np.all(base[hi:].view(np.int64) == kc.SENTINEL)
        assert ok, "a guard word next to a device vector changed: a write outside its n elements"
        return base[self.lo:hi].reshape(self.data.shape).copy()

    def unchanged(self):
        assert kc.same_bits(self.host(), self.data), "a pass wrote to one of its inputs"


_checking = [True]


def _chk(check, *args):
    """A check of krylov_pass_cases; the second of two runs of a case only compares bits with the first."""
    return check(*args) if _checking[0] else 0.0


def _place(arrays, layout):
    return [Guarded(a, kc.offset(layout, c)) for c, a in enumerate(arrays)]


def _vector_passes(mg, dev, n, layout):
    """Every vector pass once on fresh seeded vectors; returns ({name: bits}, worst ratio)."""
    D = mg.device
    res, worst = {}, 0.0
    a, b = kc.ALPHA, kc.BETA

    x, y = _place(kc.vectors(n, 2, 1), layout)
    res["dot"] = np.array([dev.kry_dot(x.v, y.v, n)])
    res["norm"] = np.array([dev.kry_norm(y.v, n)])
    ws, out = Guarded(np.zeros(1024)), Guarded(np.zeros(1))
    D.vec_sumsq(y.v, n, ws.v, out.v)
    ws.host()
    res["sumsq"] = out.host()
    worst = max(worst, _chk(kc.check_dot, "dot", res["dot"][0], x.data, y.data), _chk(kc.check_norm, "norm", res["norm"][0], y.data),
                _chk(kc.check_sumsq, "sumsq", res["sumsq"][0], y.data))
    x.unchanged(), y.unchanged()

    x, y = _place(kc.vectors(n, 2, 2), layout)
    dev.kry_axpby(a, x.v, b, y.v, n)
    res["axpby"] = y.host()
    worst = max(worst, _chk(kc.check_axpby, "axpby", res["axpby"], a, x.data, b, y.data))
    ynan = Guarded(np.full(n, np.nan), kc.offset(layout, 1))
    dev.kry_axpby(a, x.v, 0.0, ynan.v, n)                               # start_basis: V_0 = r / ||r|| into work space nobody initialised
    res["axpby0"] = ynan.host()
    assert not np.isnan(res["axpby0"]).any(), "axpby with b == 0 read y"
    worst = max(worst, _chk(kc.check_axpby, "axpby b == 0", res["axpby0"], a, x.data, 0.0, ynan.data))
    x.unchanged()

    for with_norm in (False, True):
        p, q, xx, r = _place(kc.vectors(n, 4, 3), layout)
        nrm = dev.kry_cg_update(a, p.v, q.v, xx.v, r.v, n, norm=with_norm)
        gx, gr = xx.host(), r.host()
        worst = max(worst, _chk(kc.check_cg_update, f"cg_update norm={with_norm}", gx, gr, a, p.data, q.data, xx.data, r.data, nrm))
        p.unchanged(), q.unchanged()
        res[f"cg_update{int(with_norm)}"] = np.concatenate([gx, gr, [nrm if with_norm else 0.0]])

    z, p = _place(kc.vectors(n, 2, 4), layout)
    dev.kry_cg_p(b, z.v, p.v, n)
    res["cg_p"] = p.host()
    worst = max(worst, _chk(kc.check_cg_p, "cg_p", res["cg_p"], b, z.data, p.data))
    z.unchanged()

    for with_u in (True, False):
        v, w, u = _place(kc.vectors(n, 3, 5), layout)
        hk, out = Guarded(np.array([0.77])), Guarded(np.zeros(1))
        dev.kry_mgs_step(hk.v, v.v, w.v, u.v if with_u else None, n, out.v)
        gw, go = w.host(), out.host()
        worst = max(worst, _chk(kc.check_mgs_step, f"mgs_step u={with_u}", gw, go[0], 0.77, v.data, w.data, u.data if with_u else None))
        v.unchanged(), u.unchanged(), hk.unchanged()
        res[f"mgs_step{int(with_u)}"] = np.concatenate([gw, go])

    worst = max(worst, _dscale_xpdr(mg, n, 1, layout, res))
    return res, worst


def _dscale_xpdr(mg, n, nrhs, layout, res):
    """mg_vec_dscale / xpdr on [n][nrhs] blocks; d differs in every row."""
    rng = np.random.default_rng(40 + nrhs)
    dv = rng.uniform(0.5, 1.5, n) * np.where(np.arange(n) % 2, -1.0, 1.0)
    d, bb, xx, o1, o2 = _place([dv, rng.standard_normal((n, nrhs)), rng.standard_normal((n, nrhs)), np.full((n, nrhs), np.nan),
                                np.full((n, nrhs), np.nan)], layout)
    mg.device.vec_dscale(d.v, bb.v, o1.v, n, nrhs)
    mg.device.vec_xpdr(xx.v, d.v, bb.v, o2.v, n, nrhs)
    res[f"dscale{nrhs}"], res[f"xpdr{nrhs}"] = o1.host(), o2.host()
    d.unchanged(), bb.unchanged(), xx.unchanged()
    return max(_chk(kc.check_dscale, f"dscale nrhs={nrhs}", res[f"dscale{nrhs}"], dv, bb.data),
               _chk(kc.check_xpdr, f"xpdr nrhs={nrhs}", res[f"xpdr{nrhs}"], xx.data, dv, bb.data))


def _twice(run):
    first, worst = run()
    _checking[0] = False
    try:
        second, _ = run()
    finally:
        _checking[0] = True
    for name, bits in first.items():
        assert kc.same_bits(bits, second[name]), ("two runs differ", name)
    return worst


@pytest.mark.parametrize("n", kc.VEC_N)
@pytest.mark.parametrize("layout", kc.LAYOUTS)
def test_vector_passes_vs_long_double(mg, dev, n, layout):
    worst = _twice(lambda: _vector_passes(mg, dev, n, layout))
    print(f"  n = {n}, layout {layout}: worst ratio of error to bound {worst:.3f}")


@pytest.mark.parametrize("n", kc.BLK_N)
@pytest.mark.parametrize("nrhs", kc.NRHS[1:])
@pytest.mark.parametrize("layout", kc.LAYOUTS)
def test_dscale_xpdr_blocks_vs_long_double(mg, dev, n, nrhs, layout):
    def run():
        res = {}
        return res, _dscale_xpdr(mg, n, nrhs, layout, res)
    worst = _twice(run)
    print(f"  n = {n}, nrhs = {nrhs}, layout {layout}: worst ratio of error to bound {worst:.3f}")


# ---- the Gram-Schmidt chain -----------------------------------------------------------------------------------------------------------
def _chain_tail(n):
    return min(n, 4096)          # sentinel behind w: where a chain that went one vector too far would write


def _chain(dev, V, n, i, off):
    g = Guarded(V, off, tail=_chain_tail(n))
    h = dev.kry_mgs_chain(g.v, n, i)
    return h, g.host()


def _chain_cases(n):
    return kc.CHAIN_I + ((kc.CHAIN_LAST[1],) if n == kc.CHAIN_LAST[0] else ())


@pytest.mark.parametrize("n", kc.VEC_N)
@pytest.mark.parametrize("off", [0, 1])
def test_chain_breakdown_is_exact(dev, n, off):
    """V_0 = e_1, w = 3 e_1: h_0 == 3 and ||w||^2 == 0 exactly, w comes back all zeros without a NaN (scale_rsqrt returns without
    writing when *wn2 == 0), the basis and everything behind w untouched."""
    for i in _chain_cases(n):
        V, h_exact = kc.chain_breakdown(n, i)
        h, got = _chain(dev, V, n, i, off)
        assert kc.same_bits(h, h_exact), (i, h)
        assert kc.same_bits(got[:i + 1], V[:i + 1]) and kc.same_bits(got[i + 1], np.zeros(n)), i
    print(f"  n = {n}, base {8 * off} bytes past a boundary: exact at i = {_chain_cases(n)}")


@pytest.mark.parametrize("n", kc.VEC_N)
@pytest.mark.parametrize("off", [0, 1])
def test_chain_equals_its_steps_one_by_one(dev, n, off):
    """Every mgs_step of the chain alone against long double from the device's own h_k (read back) and the vectors it was given; then
    mg_kry_mgs_chain must equal, bit for bit, the same launches issued one by one through mg_kry_dot / mg_kry_mgs_step (the closing
    scale a * w with a = 1 / sqrt(||w||^2) restated on the host: one correctly rounded product per element), and its h_host the scalars
    those calls left.  The basis vectors are n apart, so their alignment follows from the base and n alone."""
    worst = 0.0
    for i in _chain_cases(n):
        V = kc.chain_random(n, i, 50 + i)
        g = Guarded(V, off, tail=_chain_tail(n))
        hd = torch.zeros(i + 2, dtype=torch.float64, device="cuda")
        w = g.v[i + 1]
        hd[0] = dev.kry_dot(w, g.v[0], n)
        worst = max(worst, _chk(kc.check_dot, f"i={i} h_0", float(hd[0]), V[i + 1], V[0]))
        before = V[i + 1]
        for k in range(i + 1):
            dev.kry_mgs_step(hd[k:k + 1], g.v[k], w, g.v[k + 1] if k < i else None, n, hd[k + 1:k + 2])
            torch.cuda.synchronize()
            after, hs = w.cpu().numpy(), hd.cpu().numpy()
            worst = max(worst, _chk(kc.check_mgs_step, f"i={i} step {k}", after, hs[k + 1], hs[k], V[k], before, V[k + 1] if k < i else None))
            before = after
        steps = g.host()
        assert kc.same_bits(steps[:i + 1], V[:i + 1])
        hs = hd.cpu().numpy()
        assert hs[i + 1] > 0.0
        scaled = (1.0 / np.sqrt(hs[i + 1])) * steps[i + 1]
        h, got = _chain(dev, V, n, i, off)
        h2, got2 = _chain(dev, V, n, i, off)
        assert kc.same_bits(h, hs), (i, h, hs)
        assert kc.same_bits(got[:i + 1], V[:i + 1]) and kc.same_bits(got[i + 1], scaled), i
        assert kc.same_bits(h, h2) and kc.same_bits(got, got2), ("two runs differ", i)
    print(f"  n = {n}, base {8 * off} bytes past a boundary: worst ratio of error to bound {worst:.3f}")


# ---- blocks ---------------------------------------------------------------------------------------------------------------------------------
def _block_passes(dev, n, k, off):
    res, worst = {}, 0.0
    Xd, Yd, Cm = kc.block(n, k, 5), kc.block(n, k, 6), kc.coeff(k, 7)
    X, Y = Guarded(Xd, off), Guarded(Yd, off)
    res["gram"], res["gram_xx"] = dev.kry_blk_gram(X.v, Y.v, n, k), dev.kry_blk_gram(X.v, X.v, n, k)
    worst = max(worst, _chk(kc.check_gram, "gram X'Y", res["gram"], Xd, Yd), _chk(kc.check_gram, "gram X'X", res["gram_xx"], Xd, Xd))
    X.unchanged(), Y.unchanged()

    def comb(name, out, add, s, inp, add_data):
        dev.kry_blk_comb(out.v, add.v if add is not None else None, s, inp.v, Cm, n, k)
        res[name] = out.host()
        for t in (add, inp):
            if t is not None and t is not out:
                t.unchanged()
        return _chk(kc.check_comb, name, res[name], add_data, s, Xd, Cm)

    O = Guarded(np.full((n, k), np.nan), off)
    worst = max(worst, comb("comb add == NULL", O, None, 0.0, X, None))                  # blk_cholqr: W = W C with out == in below
    O = Guarded(np.full((n, k), np.nan), off)
    worst = max(worst, comb("comb all distinct", O, Y, -0.625, X, Yd))
    In = Guarded(Xd, off)
    worst = max(worst, comb("comb out == in", In, None, 0.0, In, None))
    In = Guarded(Xd, off)
    worst = max(worst, comb("comb out == in, add", In, Y, 1.0, In, Yd))                   # P = Z + P Beta
    Ad = Guarded(Yd, off)
    worst = max(worst, comb("comb out == add", Ad, Ad, 1.0, X, Yd))                       # X += P Alpha
    Yn = Yd.copy()
    Yn[::3, k // 2] = np.nan
    O, An = Guarded(np.full((n, k), np.nan), off), Guarded(Yn, off)
    worst = max(worst, comb("comb s == 0, NaN in add", O, An, 0.0, X, Yn))
    return res, worst


@pytest.mark.parametrize("n", kc.BLK_N)
@pytest.mark.parametrize("k,off", [(k, off) for k in kc.BLK_K for off in ((0, 1) if k % 2 else (0,))])
def test_block_passes_vs_long_double(dev, n, k, off):
    worst = _twice(lambda: _block_passes(dev, n, k, off))
    print(f"  n = {n}, k = {k}, {8 * off} bytes past a boundary: worst ratio of error to bound {worst:.3f}")


# ---- refusals on the device ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(mg, dev):
    D = mg.device
    lib = D.load_library()
    n = 65
    x, y = _place(kc.vectors(n, 2, 9), 0)
    blk = Guarded(kc.block(n, 16, 9))
    one = C.c_double(0.0)
    o, h, px, py, pb = C.byref(one), dev.handle, x.v.data_ptr(), y.v.data_ptr(), blk.v.data_ptr()
    torch.cuda.synchronize()
    Cm = np.zeros(17 * 17)
    cp = Cm.ctypes.data_as(C.POINTER(C.c_double))
    invalid = [lib.mg_kry_dot_dev_FP64(h, None, py, n, o), lib.mg_kry_dot_dev_FP64(h, px, py, 0, o), lib.mg_kry_norm_dev_FP64(h, None, n, o),
               lib.mg_kry_axpby_dev_FP64(h, 1.0, px, 1.0, None, n), lib.mg_kry_cg_update_dev_FP64(h, 1.0, px, None, py, py, n, None),
               lib.mg_kry_cg_p_dev_FP64(h, 1.0, None, py, n), lib.mg_kry_mgs_step_dev_FP64(h, None, px, py, None, n, py),
               lib.mg_kry_mgs_chain_dev_FP64(h, None, n, 0, cp), lib.mg_kry_mgs_chain_dev_FP64(h, pb, 5, 64, cp),
               lib.mg_kry_mgs_chain_dev_FP64(h, pb, 5, -1, cp), lib.mg_kry_blk_gram_dev_FP64(h, pb, pb, n, 0, cp),
               lib.mg_kry_blk_gram_dev_FP64(h, pb, pb, n, 17, cp), lib.mg_kry_blk_gram_dev_FP64(h, None, pb, n, 2, cp),
               lib.mg_kry_blk_comb_dev_FP64(h, pb, None, 0.0, pb, cp, n, 0), lib.mg_kry_blk_comb_dev_FP64(h, pb, None, 0.0, pb, cp, n, 17),
               lib.mg_kry_blk_comb_dev_FP64(h, pb, None, 0.0, None, cp, n, 2)]
    assert invalid == [D.MG_ERR_INVALID] * len(invalid), invalid
    raw = C.c_void_p()
    assert lib.mg_create_CF64(2, 1, 0, C.byref(raw)) == 0                    # a complex handle
    try:
        state = [lib.mg_kry_dot_dev_FP64(raw, px, py, n, o), lib.mg_kry_axpby_dev_FP64(raw, 1.0, px, 1.0, py, n),
                 lib.mg_kry_mgs_chain_dev_FP64(raw, pb, 5, 0, cp), lib.mg_kry_blk_gram_dev_FP64(raw, pb, pb, n, 2, cp)]
    finally:
        lib.mg_destroy(raw)
    assert state == [D.MG_ERR_STATE] * len(state), state
    raw = C.c_void_p()
    assert lib.mg_create(2, 1, 0, C.byref(raw)) == 0                         # a real handle that was never finalized
    try:
        assert lib.mg_kry_norm_dev_FP64(raw, px, n, o) == D.MG_ERR_STATE
    finally:
        lib.mg_destroy(raw)
    x.unchanged(), y.unchanged(), blk.unchanged()                            # nothing was launched ...
    _chk(kc.check_dot, "dot after the refusals", dev.kry_dot(x.v, y.v, n), x.data, y.data)   # ... and the handle still serves
