"""The bounds of the real Krylov drivers' kernel-level test (tests/krylov_pass_cases.py) on the CPU: for every pass a plain fp64 numpy
restatement in the kernel's order (pairs, then the tail; per-workgroup partials, then the final sum) stays inside its bound at every
shape of the GPU test, and at least one deliberately wrong variant of it falls outside - the bounds are satisfiable and tight enough
to catch what they are for.  Also: the wrappers and the header's declarations exist, and the refusals that need no device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import krylov_pass_cases as kc  # noqa: E402

ENTRIES = ("dot", "norm", "axpby", "cg_update", "cg_p", "mgs_step", "mgs_chain", "blk_gram", "blk_comb")
ODD_N = [n for n in kc.VEC_N if n % 2 == 1]
MULTI_N = [n for n in kc.VEC_N if kc.reduction_blocks(n) > 1]          # more than one workgroup's partial


def _rejected(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


@pytest.mark.parametrize("n", kc.VEC_N)
def test_reductions_inside_their_bounds(n):
    x, y = kc.vectors(n, 2, 1)
    worst = max(kc.check_dot("dot", kc.model_dot(x, y), x, y), kc.check_sumsq("sumsq", kc.model_sumsq(x), x),
                kc.check_norm("norm", kc.model_norm(x), x))
    print(f"  n = {n}: worst ratio {worst:.3e}")
    if n in ODD_N:                                                     # the odd last element dropped
        _rejected(kc.check_dot, "dot, no tail", kc.model_dot(x, x + 2.0, drop_tail=True), x, x + 2.0)
        _rejected(kc.check_sumsq, "sumsq, no tail", kc.model_sumsq(x, drop_tail=True), x)
        _rejected(kc.check_norm, "norm, no tail", kc.model_norm(x, drop_tail=True), x)
    if n in MULTI_N:                                                   # the last workgroup's partial dropped
        _rejected(kc.check_dot, "dot, a partial short", kc.model_dot(x, x + 2.0, drop_last_partial=True), x, x + 2.0)
        _rejected(kc.check_sumsq, "sumsq, a partial short", kc.model_sumsq(x, drop_last_partial=True), x)
        _rejected(kc.check_norm, "norm, a partial short", kc.model_norm(x, drop_last_partial=True), x)


def test_every_reduction_has_a_rejected_variant():
    assert ODD_N and MULTI_N and kc.CAP_N in MULTI_N and kc.reduction_blocks(kc.CAP_N) == kc.NRED_BLOCKS
    assert kc.grid_for(kc.CAP_N - 1) == kc.GRID_CAP == kc.grid_for(kc.CAP_N) and (kc.CAP_N - 1) // kc.BLK == kc.GRID_CAP


@pytest.mark.parametrize("n", kc.VEC_N)
def test_updates_inside_their_bounds(n):
    x, y, p, q = kc.vectors(n, 4, 2)
    a, b = kc.ALPHA, kc.BETA
    worst = kc.check_axpby("axpby", kc.model_axpby(a, x, b, y), a, x, b, y)
    ynan = np.full(n, np.nan)
    worst = max(worst, kc.check_axpby("axpby b == 0", kc.model_axpby(a, x, 0.0, ynan), a, x, 0.0, ynan))
    _rejected(kc.check_axpby, "axpby reads y", kc.model_axpby(a, x, 0.0, ynan, read_y=True), a, x, 0.0, ynan)
    _rejected(kc.check_axpby, "axpby b y left out", kc.model_axpby(a, x, 0.0, y), a, x, b, y)
    for with_norm in (False, True):
        xn, rn, nrm = kc.model_cg_update(a, p, q, x, y, with_norm)
        worst = max(worst, kc.check_cg_update("cg_update", xn, rn, a, p, q, x, y, nrm))
    xw, rw, _ = kc.model_cg_update(a, p, q, x, y, False, wrong_sign=True)
    _rejected(kc.check_cg_update, "cg_update r += alpha Ap", xw, rw, a, p, q, x, y)
    if min(kc.grid_for(n), kc.NRED_BLOCKS) > 1:
        xw, rw, nw = kc.model_cg_update(a, p, q, x, y, True, drop_last_partial=True)
        _rejected(kc.check_cg_update, "cg_update norm, a partial short", xw, rw, a, p, q, x, y, nw)
    worst = max(worst, kc.check_cg_p("cg_p", kc.model_cg_p(b, x, p), b, x, p))
    _rejected(kc.check_cg_p, "cg_p roles swapped", kc.model_cg_p(b, x, p, swapped=True), b, x, p)
    print(f"  n = {n}: worst ratio {worst:.3e}")


@pytest.mark.parametrize("n", kc.VEC_N)
def test_mgs_step_and_chain_inside_their_bounds(n):
    v, w, u = kc.vectors(n, 3, 3)
    hk, worst = 0.77, 0.0
    for other in (u, None):
        wn, s = kc.model_mgs_step(hk, v, w, other)
        worst = max(worst, kc.check_mgs_step("mgs_step", wn, s, hk, v, w, other))
    wn, s = kc.model_mgs_step(hk, v, w, None, old_w_in_sum=True)
    _rejected(kc.check_mgs_step, "mgs_step sums the old w", wn, s, hk, v, w, None)
    wn, s = kc.model_mgs_step(-hk, v, w, u)
    _rejected(kc.check_mgs_step, "mgs_step adds", wn, s, hk, v, w, u)
    if n in MULTI_N:
        wn, s = kc.model_mgs_step(hk, v, w, u + 2.0 * w, drop_last_partial=True)
        _rejected(kc.check_mgs_step, "mgs_step, a partial short", wn, s, hk, v, w, u + 2.0 * w)
    for i in kc.CHAIN_I + ((kc.CHAIN_LAST[1],) if n == kc.CHAIN_LAST[0] else ()):
        V, h_exact = kc.chain_breakdown(n, i)
        h = kc.model_chain(V, i)
        assert kc.same_bits(h, h_exact) and not V[i + 1].any(), ("breakdown", n, i)      # h_0 == 3, ||w||^2 == 0, w == 0: exact
        V, _ = kc.chain_breakdown(n, i)
        kc.model_chain(V, i, divide_by_zero=True)
        assert np.isnan(V[i + 1]).all()                                                   # what scale_rsqrt's early return keeps out
    print(f"  n = {n}: worst ratio {worst:.3e}")


@pytest.mark.parametrize("nrhs", kc.NRHS)
def test_dscale_xpdr_inside_their_bounds(nrhs):
    worst = 0.0
    for n in (kc.VEC_N if nrhs == 1 else kc.BLK_N):
        rng = np.random.default_rng(40 + nrhs)
        d, b, x = rng.uniform(0.5, 1.5, n) * np.where(np.arange(n) % 2, -1.0, 1.0), rng.standard_normal((n, nrhs)), rng.standard_normal((n, nrhs))
        worst = max(worst, kc.check_dscale(f"dscale n={n}", kc.model_dscale(d, b), d, b), kc.check_xpdr(f"xpdr n={n}", kc.model_xpdr(x, d, b), x, d, b))
        if nrhs == 1 and n % 2 == 1:
            _rejected(kc.check_dscale, "dscale, no tail", kc.model_dscale(d, b, drop_tail=True), d, b)
            _rejected(kc.check_xpdr, "xpdr, no tail", kc.model_xpdr(x, d, b, drop_tail=True), x, d, b)
        if nrhs % 2 == 0 and n > 1:                                    # d taken by pair index / nrhs, not / (nrhs / 2): the wrong row
            _rejected(kc.check_dscale, "dscale, wrong row of d", kc.model_dscale(d, b, row_by_pair=True), d, b)
            _rejected(kc.check_xpdr, "xpdr, wrong row of d", kc.model_xpdr(x, d, b, row_by_pair=True), x, d, b)
    print(f"  nrhs = {nrhs}: worst ratio {worst:.3e}")


@pytest.mark.parametrize("k", kc.BLK_K)
@pytest.mark.parametrize("n", kc.BLK_N)
def test_block_passes_inside_their_bounds(n, k):
    X, Y, Cm = kc.block(n, k, 5), kc.block(n, k, 6), kc.coeff(k, 7)
    worst = kc.check_gram("gram", kc.model_gram(X, Y), X, Y)
    if k > 1:
        _rejected(kc.check_gram, "gram, a column shifted", kc.model_gram(X, Y + 1.0, shift_column=True), X, Y + 1.0)
        if n > 1:
            _rejected(kc.check_comb, "comb, C transposed", kc.model_comb(Y, 1.0, X, Cm, transposed=True), Y, 1.0, X, Cm)
            _rejected(kc.check_comb, "comb, out == in written through", kc.model_comb(None, 0.0, X, Cm, write_through=True), None, 0.0, X, Cm)
    if n > kc.BLK:
        _rejected(kc.check_gram, "gram, a partial short", kc.model_gram(X, X, drop_last_partial=True), X, X)
    for add, s in ((None, 0.0), (Y, 1.0), (Y, -0.625)):
        worst = max(worst, kc.check_comb("comb", kc.model_comb(add, s, X, Cm), add, s, X, Cm))
    Yn = Y.copy()
    Yn[::3, k // 2] = np.nan                                           # s == 0: the kernel multiplies, NaN comes through where add holds it
    worst = max(worst, kc.check_comb("comb, NaN in add", kc.model_comb(Yn, 0.0, X, Cm), Yn, 0.0, X, Cm))
    _rejected(kc.check_comb, "comb skips add at s == 0", kc.model_comb(None, 0.0, X, Cm), Yn, 0.0, X, Cm)
    _rejected(kc.check_comb, "comb, s add left out", kc.model_comb(None, 0.0, X, Cm), Y, 1.0, X, Cm)
    print(f"  n = {n}, k = {k}: worst ratio {worst:.3e}")


def test_coefficients_have_no_symmetry():
    for k in kc.BLK_K[1:]:
        Cm = kc.coeff(k, 7)
        assert np.all((Cm != Cm.T)[~np.eye(k, dtype=bool)])


# ---- the entry points: declared, bound, refusing without a device ----------------------------------------------------------------------
def test_entries_declared_and_bound(mg, built):
    header = open(os.path.join(ROOT, "include", "mgvcycle.h")).read()
    assert "the real drivers' passes on their own" in header
    lib = ctypes.CDLL(mg.device.LIB_PATH)
    for e in ENTRIES:
        name = f"mg_kry_{e}_dev_FP64"
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(lib, name) and name in mg.device.SIGNATURES, name
        assert callable(getattr(mg.device.DeviceHierarchy, f"kry_{e}")), e
    for name in ("vec_dscale", "vec_xpdr", "vec_sumsq"):
        assert callable(getattr(mg.device, name))


def test_null_handle_is_refused_without_a_device(mg, built):
    """A null handle is MG_ERR_INVALID before anything touches a device."""
    lib = mg.device.load_library()
    one = ctypes.c_double(0.0)
    o = ctypes.byref(one)
    calls = {"dot": (None, 8, 8, 1, o), "norm": (None, 8, 1, o), "axpby": (None, 1.0, 8, 0.0, 8, 1), "cg_update": (None, 1.0, 8, 8, 8, 8, 1, None),
             "cg_p": (None, 1.0, 8, 8, 1), "mgs_step": (None, 8, 8, 8, None, 1, 8), "mgs_chain": (None, 8, 1, 0, o),
             "blk_gram": (None, 8, 8, 1, 1, o), "blk_comb": (None, 8, None, 0.0, 8, o, 1, 1)}
    assert sorted(calls) == sorted(ENTRIES)
    for e, args in calls.items():
        rc = getattr(lib, f"mg_kry_{e}_dev_FP64")(*args)
        assert rc == mg.device.MG_ERR_INVALID, (e, rc)
        assert b"null hierarchy handle" in lib.mg_last_error(), e
