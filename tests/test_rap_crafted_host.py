"""CPU: the checks of tests/rap_crafted_cases.py against plain restatements of the device re-setup's kernels - the product in the
kernels' own order (R in stored order, A in stored order and by lane groups, one row of P per step, the group copies summed in
order) must stay inside the entry bound on both levels and for every value type, the exact family must come out bit for bit - and
against wrong variants of them, each of which must leave the bound in an entry named here.

Largest share of a bound the restatement uses (printed by test_restatement_stays_inside_the_bound; unfused double arithmetic):
float64 0.62 (level 1 -> 2) / 0.16 (2 -> 3); complex128 0.22 / 0.04 with one group, 0.08 / 0.02 with 8; complex64 1.00 / 0.98 - the rounding to single
is half an ulp of single wherever the double sum falls midway, and the bound grants exactly that.  The exact family: 0 everywhere.

The 2^-40 perturbation (test_a_relative_change_of_2_to_the_minus_40_is_seen): every entry of one or two terms without cancellation
leaves its bound; from m + 2 >= 2^13 (complex: m + groups + 1 >= 2896) on it cannot be seen - the crafted hierarchy's largest m is 14 on
level 1 -> 2 and 702 on level 2 -> 3, so all of its entries whose terms do not cancel are covered."""
import numpy as np
import pytest

import rap_crafted_cases as K

GROUPS = {"float64": (1,), "complex128": (1, 2, 8, 16), "complex64": (1, 8)}


def _level_values(vt, family, groups):
    """[(T, R, A, P)] of both levels; level 2's A is the restatement's own level-2 result (as the device's is on the device)."""
    H, v = K.hierarchy(), K.values(vt, family)
    A2 = K.kernel_order(vt, H["T"][0], v["R"][0], v["A"], v["P"][0], groups=groups)
    return [(H["T"][0], v["R"][0], v["A"], v["P"][0]), (H["T"][1], v["R"][1], A2, v["P"][1])]


def test_the_hierarchy_holds_the_shapes_it_is_there_for():
    H = K.hierarchy()
    assert [M.shape[0] for M in H["A"]] + [H["C"][1].shape[0]] == [K.N1, K.N2, K.N3]
    assert H["C"][0].lens.max() == 4100 and H["T"][0].m.max() >= 8 and H["T"][1].m.max() >= 500
    assert K.lane_groups(0, 2048, 4100) == 1 and K.lane_groups(0, 10, 4100) == 8 and K.lane_groups(16, 5000, 40) == 16
    assert K.lane_groups(3, 1, 40) == 2 and K.lane_groups(16, 2048, 300) == 4


@pytest.mark.parametrize("family", ["crafted", "exact"])
@pytest.mark.parametrize("vt", K.VTYPES)
def test_restatement_stays_inside_the_bound(vt, family):
    for groups in GROUPS[vt]:
        for lvl, (T, R, A, P) in enumerate(_level_values(vt, family, groups), 1):
            got = K.kernel_order(vt, T, R, A, P, groups=groups)
            share = K.check_entries(f"{vt} {family} level {lvl} -> {lvl + 1}, {groups} groups", vt, T, got, K.reference(T, R, A, P),
                                    groups=groups, exact=family == "exact")
            print(f"\n{vt} {family} level {lvl} -> {lvl + 1}, {groups} groups: largest share of a bound {share:.3f}")
            assert (got[T.m == 0] == 0).all()


def _case(vt, groups=None):
    groups = (1 if vt == "float64" else 8) if groups is None else groups
    H, v = K.hierarchy(), K.values(vt, "crafted")
    T, R, A, P = H["T"][0], v["R"][0], v["A"], v["P"][0]
    return H, T, (R, A, P), K.reference(T, R, A, P), groups


def _row_entries(H, name):
    C, i = H["C"][0], H["marks"][name]
    return int(C.indptr[i]), int(C.indptr[i + 1])


@pytest.mark.parametrize("vt", K.VTYPES)
def test_wrong_products_leave_the_bound_in_a_named_entry(vt):
    H, T, (R, A, P), ref, groups = _case(vt)
    run = lambda **kw: K.kernel_order(vt, T, R, A, P, groups=groups, **kw)
    out = lambda got: set(K.outside(vt, T, got, ref, groups).tolist())
    assert not out(run())
    s, e = _row_entries(H, "len4097")
    two = s + int(np.flatnonzero(T.m[s:e] == 2)[0])                       # an entry of two terms in the 4097-entry row
    first = int(np.searchsorted(T.pos, two))
    # one term dropped / added twice
    w = np.ones(T.pos.size)
    w[first + 1] = 0.0
    assert two in out(run(weight=w)), T.name(two)
    w[first + 1] = 2.0
    assert two in out(run(weight=w)), T.name(two)
    big = int(np.argmax(T.m))                                             # ... and in the entry of the most terms
    w = np.ones(T.pos.size)
    w[int(np.searchsorted(T.pos, big)) + 3] = 0.0
    assert big in out(run(weight=w)), T.name(big)
    # the entries of a row of P beyond the first lane trip dropped
    W = 64 // groups
    beyond = np.unique(T.pos[T.poff >= W])
    assert beyond.size > 100
    missed = out(run(first_trip=W))
    named = int(beyond[0])
    assert named in missed and set(beyond.tolist()) <= missed, T.name(named)
    # the last chunk of a row left at zero
    for name, length in (("len2049", 2049), ("len4097", 4097)):
        s, e = _row_entries(H, name)
        got = run()
        last = s + (length - 1) // K.RAP_CAP * K.RAP_CAP
        got[last:e] = 0
        assert set(range(last, e)) <= out(got), T.name(last)
    # a chunk-boundary column credited to the neighbouring chunk
    s, e = _row_entries(H, "len2049")
    pos = T.pos.copy()
    pos[pos == s + 2048] = s + 2047
    assert {s + 2047, s + 2048} <= out(run(pos=pos)), (T.name(s + 2047), T.name(s + 2048))
    # one group copy not summed
    if groups > 1:
        in3 = np.unique(T.pos[T.goff % groups == 3])
        missed = out(run(skip_group=3))
        assert in3.size > 100 and int(in3[0]) in missed and set(in3.tolist()) <= missed, T.name(int(in3[0]))
    # an unreachable structural entry keeping its previous value
    s, e = _row_entries(H, "holes")
    for hole in (s, s + 2047, s + 2048, e - 1, _row_entries(H, "empty_R")[0]):
        assert T.m[hole] == 0
        for old in (np.nan, 1e-30, -0.5):
            got = run()
            got[hole] = old
            assert hole in out(got), (T.name(hole), old)
        got = run()
        got[hole] = -0.0                                                  # ... or coming back as -0.0
        with pytest.raises(AssertionError, match="is -0.0"):
            K.check_entries("minus zero", vt, T, got, ref, groups)


@pytest.mark.parametrize("vt", ["float64", "complex128"])
def test_a_relative_change_of_2_to_the_minus_40_is_seen(vt):
    H, T, (R, A, P), ref, groups = _case(vt)
    got = K.kernel_order(vt, T, R, A, P, groups=groups) * (1.0 + 2.0 ** -40)
    missed = np.zeros(T.nnz, dtype=bool)
    missed[K.outside(vt, T, got, ref, groups)] = True
    mag = np.hypot(ref[0], ref[1]).astype(np.float64)
    plain = (T.m > 0) & (mag >= 0.5 * ref[2])                    # entries whose terms do not cancel (|ref| >= sum|t| / 2)
    assert plain.sum() > 0.5 * T.nnz and missed[plain].all() and missed[(T.m == 1) | (T.m == 2) & plain].all()
    # where it stops: gamma(m + 2) >= 2^-40 from m + 2 = 2^13 on (complex: (m + groups + 1) u_c >= 2^-40 from 2896 on)
    assert K.gamma(2 ** 13) >= 2.0 ** -40 > K.gamma(2 ** 13 - 1) and K.gamma_c(2897) >= 2.0 ** -40 > K.gamma_c(2895)
    s, e = _row_entries(H, "cancel")
    assert not missed[s + 1] or vt == "complex64"                # (the entry that cancels to 2^-40 hides it: |ref| = 2^-41 sum|t|)


@pytest.mark.parametrize("vt", K.VTYPES)
def test_relaxation_vectors_and_their_wrong_variants(vt):
    H, v = K.hierarchy(), K.values(vt, "crafted")
    LD = K.LD
    for pat, val in ((H["A"][0], v["A"]), (H["A"][1], K.kernel_order(vt, H["T"][0], v["R"][0], v["A"], v["P"][0]))):
        w = K._wide(val)
        diag = K._diag(pat, val)
        has = np.zeros(pat.shape[0], dtype=bool)
        has[pat.rows[pat.indices == pat.rows]] = True
        # the restated vectors against the same in long double (Jac: two roundings and a division; SPAI: k + 2 roundings)
        s = K.colsumsq(vt, pat, val)
        sq = (w.real.astype(LD) ** 2 + w.imag.astype(LD) ** 2)
        s_ld = np.zeros(pat.shape[1], dtype=LD)
        np.add.at(s_ld, pat.indices, sq)
        k = np.bincount(pat.indices, minlength=pat.shape[1])
        assert (np.abs(s.astype(LD) - s_ld) <= K.gamma(k + 2) * s_ld).all()
        ok = has & (s > 0)
        d = K.spai(vt, pat, val)
        want = K.OMEGA * np.conj(diag[ok]).astype(np.clongdouble if np.iscomplexobj(diag) else LD) / s_ld[ok]
        tol = (K.gamma(k[ok] + 4) + (K.U32 if vt == "complex64" else 0)) * np.abs(want).astype(np.float64) * np.sqrt(2)
        assert (np.abs(d[ok] - want) <= tol).all()
        nz = has & (np.abs(diag) > 0)
        for j in K.jacobi(vt, pat, val):
            wantj = K.OMEGA / diag[nz].astype(np.clongdouble if np.iscomplexobj(diag) else LD)
            assert (np.abs(j[nz] - wantj) <= (K.gamma(6) * 2 + (K.U32 if vt == "complex64" else 0)) * np.abs(wantj).astype(np.float64) * 2).all()
        K.check_relax("restated Jac", vt, 0, pat, val, K.jacobi(vt, pat, val)[-1])
        K.check_relax("restated SPAI", vt, 1, pat, val, d)
        # the wrong variants
        with pytest.raises(AssertionError):
            K.check_relax("rows for columns", vt, 1, pat, val, K.spai(vt, pat, val, over_rows=True))
        if vt != "float64":
            with pytest.raises(AssertionError):
                K.check_relax("conj missing", vt, 1, pat, val, K.spai(vt, pat, val, conj=False))
        with pytest.raises(AssertionError):
            K.check_relax("one ulp", vt, 0, pat, val, np.nextafter(K.jacobi(vt, pat, val)[0].real, np.inf).astype(K.rdtype(vt))
                          + (1j * K.jacobi(vt, pat, val)[0].imag if vt != "float64" else 0))
    A1 = H["A"][0]
    cols = np.bincount(A1.indices, minlength=K.N1)
    assert sorted(cols[list(K.COL_LENS)]) == [1, 2, 64, 65, 3000]
