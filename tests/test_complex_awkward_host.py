"""No GPU: the references and bounds of tests/complex_awkward_cases.py are fit to judge a kernel.  The plain numpy cycle in the working
precision (tests/complex_oracle.py in complex128, tests/complex_single_oracle.py in complex64 on the rounded data) is held against
the long-double references: it must use at most a quarter of every row's sweep bound (a bound that plain arithmetic uses up cannot
tell a wrong kernel from rounding), stay within 1e-14 of the long-double full cycle (1 % of the project's 1e-12 cycle tolerance) and,
in single, below 64 * 2^-24 in the 2-norm.  The operator must cut every row-block class the kernels have an edge path for, and a
relative error of 1e-13 in one row must leave the row-wise bound while it stays far below a 1e-12 max-norm comparison."""
import numpy as np
import pytest

import complex_awkward_cases as ac
import complex_oracle as corc
import complex_single_oracle as cs


def test_the_operator_cuts_every_row_block_class():
    A = ac.awkward6007()
    assert A.shape == (ac.N, ac.N) and ac.N % ac.MAXROWS != 0 and A.has_sorted_indices
    lens = np.diff(A.indptr)
    assert lens[2500] == ac.CX_CHUNK and lens[2501] == ac.CX_CHUNK + 1 and lens[2000] == 3000 and lens[-1] == 900
    assert not lens[3100:3400].any() and (lens == 0).sum() >= 340
    c = ac.block_classes(A.indptr)
    print(f"  {c['nblocks']} row blocks: {len(c['full_empty'])} of {ac.MAXROWS} empty rows, {len(c['full'])} of {ac.MAXROWS} rows with entries, "
          f"{len(c['exact_chunk'])} one-row of exactly {ac.CX_CHUNK}, {len(c['long_row'])} long rows, {len(c['nearly_full'])} multi-row "
          f"of >= 1000 entries, last block a single row: {c['last_single']}")
    assert len(c["full_empty"]) >= 1
    assert len(c["full"]) >= 1
    assert len(c["exact_chunk"]) == 1
    assert len(c["long_row"]) == 2
    assert len(c["nearly_full"]) >= 1
    assert c["last_single"]
    blk = ac.row_blocks(A.indptr)                    # the partition covers the rows once, within both limits
    assert blk[0] == 0 and blk[-1] == ac.N and np.all(np.diff(blk) >= 1) and np.all(np.diff(blk) <= ac.MAXROWS)
    nnz = A.indptr[blk[1:]] - A.indptr[blk[:-1]]
    assert np.all((nnz <= ac.CX_CHUNK) | (np.diff(blk) == 1))
    for kind in ("full", "sweeps"):                  # the transfer operators: every fine row read by R and written by P
        h = ac.hierarchy(kind, False)
        assert np.all(np.diff(h.P.indptr) == 1) and np.all(np.diff(h.R.tocsc().indptr) == 1) and h.Ac.shape == (ac.NC, ac.NC)
    assert not ac.hierarchy("sweeps", False).P.data.any() and not ac.hierarchy("sweeps", True).P.data.any()
    assert np.array_equal(ac.hierarchy("sweeps", False).P.indices, ac.hierarchy("full", False).P.indices)


def _plain_cycle(mg, h, b, x0, pre, post, from_zero):
    p = h.param(mg, pre, post)
    x = np.zeros_like(b) if from_zero else x0.copy()
    return (cs if h.single else corc).recursiveCycle(p, b.copy(), x, 1)


@pytest.mark.parametrize("single", [False, True])
def test_plain_sweeps_use_a_quarter_of_the_bound(mg, single):
    h = ac.hierarchy("sweeps", single)
    b, x0 = ac.vector(1, single), ac.vector(2, single)
    worst, rel = 0.0, []
    for pre, post in ac.SWEEPS_HOST:
        for from_zero in (True, False):
            ref = ac.sweep_chain(h, b, x0, pre, post, from_zero)
            assert np.array_equal(ref, ac.ld_cycle(h, b, x0, pre, post, from_zero))      # the coarse correction adds exact zeros
            E = ac.sweep_bound(h, b, x0, pre, post, from_zero)
            got = _plain_cycle(mg, h, b, x0, pre, post, from_zero)
            assert got.dtype == h.cdtype
            r = ac.within_rows(got, ref, E, 0.25)
            rel.append(float(np.median(E / np.abs(ref).astype(np.float64))))
            assert float(np.abs(ref).max()) < 40.0                                       # the chain is a well-conditioned map
            worst = max(worst, r)
    print(f"  sweeps, {'single' if single else 'double'}: worst row ratio of the plain numpy cycle {worst:.3f}; median E/|x| "
          f"{min(rel):.1e} to {max(rel):.1e}")


def test_plain_full_cycle_against_long_double(mg):
    h = ac.hierarchy("full", False)
    b = ac.vector(1, False)
    worst = 0.0
    for pre, post in ac.SWEEPS_HOST:
        x = _plain_cycle(mg, h, b, None, pre, post, True)
        ref = ac.ld_cycle(h, b, None, pre, post, True)
        e1 = float(np.abs(x.astype(ac.CLD) - ref).max() / np.abs(ref).max())
        x2 = _plain_cycle(mg, h, b, x, pre, post, False)
        ref2 = ac.ld_cycle(h, b, x, pre, post, False)
        e2 = float(np.abs(x2.astype(ac.CLD) - ref2).max() / np.abs(ref2).max())
        worst = max(worst, e1, e2)
        assert e1 <= 1e-14 and e2 <= 1e-14, (pre, post, e1, e2)
    print(f"  full, double: the oracle's distance from the long-double cycle {worst:.2e} in the max norm (allowed 1e-14)")


def test_plain_full_cycle_single_against_long_double(mg):
    h = ac.hierarchy("full", True)
    b = ac.vector(1, True)
    worst = 0.0
    for pre, post in ac.SWEEPS_HOST:
        x = _plain_cycle(mg, h, b, None, pre, post, True)
        e1 = cs.rel2(x, ac.ld_cycle(h, b, None, pre, post, True).astype(np.complex128))
        x2 = _plain_cycle(mg, h, b, x, pre, post, False)
        e2 = cs.rel2(x2, ac.ld_cycle(h, b, x, pre, post, False).astype(np.complex128))
        worst = max(worst, e1, e2)
        assert e1 < 64 * ac.U32 and e2 < 64 * ac.U32, (pre, post, e1, e2)
    print(f"  full, single: the restatement's distance from the long-double cycle {worst:.2e} in the 2-norm (allowed {64 * ac.U32:.2e})")


def test_a_relative_error_of_1e_13_in_one_row_leaves_the_bound():
    """The mutation check on S(d.*b), the (1, 1) cycle from zero.  A short row scaled by 1 + 1e-13 leaves its bound (35 times over)
    while the vector stays within 1e-14 of the reference in the max norm: the reason for the row-wise form.

    The long row (3000 entries) scaled by 1 + 1e-13 does NOT leave its bound, and no valid bound lets it: the row's sum alone may
    be off by gamma(3003) = 9.4e-13 relative to sum |a||x|.  Measured: the mutation is 0.0036 of the row's bound; the row resolves a
    relative error of 2.8e-11.  What is asserted for it is what the arithmetic allows: the bound is no tighter than gamma(k + 3) |x|,
    it is no looser than 64 gamma(k + 3) |x| (the row's own condition sum |a||x| / |sum a x| ~ sqrt(k) is the rest), and an error of
    twice the bound is caught."""
    h = ac.hierarchy("sweeps", False)
    b = ac.vector(1, False)
    ref = ac.sweep_chain(h, b, None, 1, 1, True)
    E = ac.sweep_bound(h, b, None, 1, 1, True)
    clean = ref.astype(np.complex128)
    assert ac.check_rows("clean", clean, ref, E) < 0.25                # the reference rounded to double is inside
    short = int(np.flatnonzero(h.rowlen == 5)[0])
    got = clean.copy()
    got[short] *= 1.0 + 1e-13
    dist = float(np.abs(got - clean).max() / np.abs(clean).max())
    assert dist < 1e-12                                                 # a max-norm comparison at 1e-12 lets it pass
    with pytest.raises(AssertionError, match="outside the componentwise bound"):
        ac.check_rows("short", got, ref, E)
    ratio = float(np.abs(got[short].astype(ac.CLD) - ref[short]) / E[short])
    print(f"  the short row {short} ({h.rowlen[short]} entries) scaled by 1 + 1e-13: {ratio:.1f} of its bound, {dist:.1e} in the max norm")
    for row in (2000, 2501):                                            # the long rows
        k = int(h.rowlen[row])
        resolves = float(E[row] / np.abs(clean[row]))
        g = float(ac.gamma(k + 3, ac.U64))
        got = clean.copy()
        got[row] *= 1.0 + 1e-13
        ratio = float(np.abs(got[row].astype(ac.CLD) - ref[row]) / E[row])
        print(f"  the long row {row} ({k} entries) scaled by 1 + 1e-13: {ratio:.4f} of its bound; gamma(k + 3) = {g:.2e}, the row "
              f"resolves a relative error of {resolves:.2e}")
        assert g > 1e-13 and g <= resolves <= 64 * g
        got = clean.copy()
        got[row] *= 1.0 + 2.0 * resolves
        with pytest.raises(AssertionError, match="outside the componentwise bound"):
            ac.check_rows("long", got, ref, E)
    got = clean.copy()
    got[7] = np.nan
    with pytest.raises(AssertionError, match="outside the componentwise bound"):
        ac.check_rows("nan", got, ref, E)


def test_norm_reference_and_bound():
    """numpy's own norm of b - A x uses a small part of the derived bound, which stays near 1e-11 relative in double."""
    h = ac.hierarchy("full", False)
    b, x = ac.vector(1, False), ac.vector(2, False)
    ref, bound = ac.residual_norm(h, b, x)
    got = float(np.linalg.norm(b - h.A @ x))
    print(f"  ||b - A x||: relative bound {bound / ref:.2e}, numpy uses {abs(got - ref) / bound:.1e} of it")
    assert abs(got - ref) <= 0.01 * bound and bound / ref < 1e-10
    ref0, bound0 = ac.residual_norm(h, b)
    assert abs(float(np.linalg.norm(b)) - ref0) <= bound0 and bound0 / ref0 < 1e-11
    B, X = ac.block(1, False, 5), ac.block(2, False, 5)
    refb, boundb = ac.residual_norm(h, B, X)
    assert abs(float(np.linalg.norm(B - h.A @ X)) - refb) <= 0.01 * boundb
