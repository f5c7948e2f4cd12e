"""-m gpu: the stand-alone factor applier (mg_lu_*_FP64, mg_lu_*_CFP64) on the crafted factors of tests/lu_crafted_cases.py, entry by
entry against the long-double reference and the derived bound (see the cases file for both; tests/test_lu_crafted_host.py shows that
plain double arithmetic uses at most a quarter of that bound and that a dropped entry, a wrong stride or a wrong start leave it).
Handles are created straight through the C ABI from the hand-made arrays; the environment is read at create, so it selects the form:
the single workgroup (sptrsv_lu), the chip-wide form without a trailing block, and the chip-wide form with a trailing block of exactly
M - mg_lu_form must confirm what ran.  One handle per configuration solves nrhs 1 .. 9 through the host entry (column-major), each
after a solve of the same width with a right-hand side 1e6 times as large (work vectors are never clean), then once more (the same
bits), nrhs = 5 also through the device entry (row-major, the same bits); b is never written."""
import ctypes as C

import numpy as np
import pytest

import lu_crafted_cases as lc

pytestmark = pytest.mark.gpu

MG_OK = 0
FORMS = {"single": {"MG_LU_MULTI_MIN_ROWS": "1000000000"},
         "wide": {"MG_LU_MULTI_MIN_ROWS": "0", "MG_LU_DENSE_TAIL_MAX": "0"}}
_worst = {}


def _tail_env(M):
    return {"MG_LU_MULTI_MIN_ROWS": "0", "MG_LU_DENSE_TAIL_MIN": str(M), "MG_LU_DENSE_TAIL_MAX": str(M)}


class Handle:
    def __init__(self, mg, c, env, monkeypatch):
        for k in ("MG_LU_MULTI_MIN_ROWS", "MG_LU_DENSE_TAIL_MIN", "MG_LU_DENSE_TAIL_MAX"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():                     # (stays set for the test: the transposed set is created on its first use)
            monkeypatch.setenv(k, v)
        self.lib, self.c = mg.device.load_library(), c
        self.I, self.F = mg.device._i64, mg.device._f64
        G = c.abi()
        self.h = C.c_void_p()
        create = self.lib.mg_lu_create_CFP64_INT64 if c.cx else self.lib.mg_lu_create_FP64_INT64
        rc = create(0, c.n, self.I(G["Lp"]), self.I(G["Lc"]), self.F(G["Lv"]), self.I(G["Up"]), self.I(G["Uc"]), self.F(G["Uv"]),
                    self.I(G["p"]), self.I(G["q"]), C.byref(self.h))
        assert rc == MG_OK, self.lib.mg_last_error()

    def form(self, t):
        info = np.zeros(7, dtype=np.int64)
        assert self.lib.mg_lu_form(self.h, t, self.I(info)) == MG_OK, self.lib.mg_last_error()
        return dict(complex=int(info[0]), multi=int(info[1]), tail=int(info[2]), launchedL=int(info[3]), launchedU=int(info[4]),
                    levelsL=int(info[5]), levelsU=int(info[6]))

    def solve(self, B, t):
        """Host entry: B (n, k) in any order -> X (n, k); column-major across the ABI; b must come back untouched."""
        Bf = np.asfortranarray(B)
        keep = Bf.copy()
        Xf = np.full(Bf.shape, np.nan, dtype=Bf.dtype, order="F")
        fn = self.lib.mg_lu_solve_CFP64 if self.c.cx else self.lib.mg_lu_solve_FP64
        assert fn(self.h, self.F(Bf), self.F(Xf), self.c.n, Bf.shape[1], t) == MG_OK, self.lib.mg_last_error()
        assert np.array_equal(Bf, keep), "the solve wrote into b"
        return Xf

    def solve_dev(self, B, t):
        """Device entry: row-major [n][k] in HBM."""
        import torch
        Bc = np.ascontiguousarray(B)
        bt = torch.from_numpy(Bc.view(np.float64).copy()).cuda()
        xt = torch.full_like(bt, float("nan"))
        torch.cuda.synchronize()
        fn = self.lib.mg_lu_solve_dev_CFP64 if self.c.cx else self.lib.mg_lu_solve_dev_FP64
        assert fn(self.h, bt.data_ptr(), xt.data_ptr(), self.c.n, Bc.shape[1], t) == MG_OK, self.lib.mg_last_error()
        torch.cuda.synchronize()
        assert np.array_equal(bt.cpu().numpy().view(Bc.dtype), Bc), "the solve wrote into b"
        return xt.cpu().numpy().view(Bc.dtype)

    def close(self):
        assert self.lib.mg_lu_destroy(self.h) == MG_OK


def _run(mg, c, env, t, monkeypatch, expect):
    """Every nrhs of lc.NRHS on one handle; returns the worst share of the bound (None for an ``exact`` case)."""
    H = Handle(mg, c, env, monkeypatch)
    try:
        f = H.form(t)
        assert f["complex"] == int(c.cx)
        expect(f)
        B = c.rhs()
        if c.exact:
            ref, E = lc.exact_solution(c, t), None
        else:
            ref, E = lc.reference(c, t)
        worst = 0.0
        for k in lc.NRHS:
            H.solve(-1.0e6 * B[:, :k], t)           # leaves large values in the work vectors: a solve that reads a stale one is seen
            X = H.solve(B[:, :k], t)
            if c.exact:
                assert np.array_equal(X, ref[:, :k]), f"{c.name} nrhs={k}: {int((X != ref[:, :k]).sum())} entries differ from the integers"
            else:
                worst = max(worst, lc.check(f"{c.name} cx={c.cx} doTranspose={t} nrhs={k}", X, ref[:, :k], E[:, :k]))
            assert np.array_equal(H.solve(B[:, :k], t), X), "a second solve gives other bits"
            if k == 5:
                assert np.array_equal(H.solve_dev(B[:, :k], t), X), "the device entry differs from the host entry"
        assert H.form(t) == f
        return None if c.exact else worst
    finally:
        H.close()


def _record(family, form, c, t, worst):
    key = (family, form, "complex" if c.cx else "real")
    _worst[key] = max(_worst.get(key, 0.0), worst)
    print(f"  {c.name} {form} {key[2]} doTranspose={t}: worst entry {worst:.3f} of its bound; so far for {key}: {_worst[key]:.3f}")


@pytest.mark.parametrize("t", [0, 1])
@pytest.mark.parametrize("form", ["single", "wide"])
@pytest.mark.parametrize("cx", [True, False])
def test_levels(mg, built, cx, form, t, monkeypatch):
    c = lc.case("levels", cx)
    lo, up = c.factors(t)[:2]

    def expect(f):
        assert f["multi"] == int(form == "wide") and f["tail"] == 0
        assert f["levelsL"] == len(lc.level_sizes(lo)) and f["levelsU"] == len(lc.level_sizes(up))
        assert f["launchedL"] == f["levelsL"] and f["launchedU"] == f["levelsU"]

    _record("levels", form, c, t, _run(mg, c, FORMS[form], t, monkeypatch, expect))


def _expect_tail(c, t):
    lo, up = c.factors(t)[:2]

    def expect(f):
        assert f["multi"] == 1 and f["tail"] == c.M, f"the trailing block is {f['tail']}, not {c.M}"
        assert f["levelsL"] == len(lc.level_sizes(lo)) and f["levelsU"] == len(lc.level_sizes(up))
        assert f["launchedL"] == len(lc.level_sizes(lo, c.M)) < f["levelsL"]
        assert f["launchedU"] == len(lc.level_sizes(up, c.M)) < f["levelsU"]
    return expect


@pytest.mark.parametrize("t", [0, 1])
@pytest.mark.parametrize("cx", [True, False])
@pytest.mark.parametrize("M", lc.TAILS)
def test_tail(mg, built, M, cx, t, monkeypatch):
    c = lc.case(f"tail{M}", cx)
    _record("tail", "wide", c, t, _run(mg, c, _tail_env(M), t, monkeypatch, _expect_tail(c, t)))


@pytest.mark.parametrize("t", [0, 1])
@pytest.mark.parametrize("cx", [True, False])
@pytest.mark.parametrize("form", ["single", "wide"])
def test_exact_levels(mg, built, form, cx, t, monkeypatch):
    c = lc.case("exact_levels", cx)

    def expect(f):
        assert f["multi"] == int(form == "wide") and f["tail"] == 0 and f["launchedL"] == f["levelsL"]

    assert _run(mg, c, FORMS[form], t, monkeypatch, expect) is None


@pytest.mark.parametrize("t", [0, 1])
@pytest.mark.parametrize("cx", [True, False])
@pytest.mark.parametrize("M", lc.EXACT_TAILS)
def test_exact_tail(mg, built, M, cx, t, monkeypatch):
    c = lc.case(f"exact_tail{M}", cx)
    assert _run(mg, c, _tail_env(M), t, monkeypatch, _expect_tail(c, t)) is None
