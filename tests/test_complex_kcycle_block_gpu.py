"""-m gpu: blocks of right-hand sides on K-cycle / Jac-GMRES complex hierarchies (``blockKcycle=True``; the handle's option
kcycle_blocks, mg_block_fgmres_relax_CF64 / _CF32, the GRAM mode of cx_csr_stream_spmm, its fronts and the flat combination pass) on the
MI355X, against numpy on the device's own bases and against the Kronecker oracle of tests/complex_kcycle_block_cases.py (the existing
tests/complex_kcycle_oracle.py on kron(A, I_k): the reference's long-vector form).  The conditions on the inputs are asserted by
tests/test_complex_kcycle_block_host.py and, where a comparison depends on one, once more here on the oracle alone.

Tolerances.
  * AZ_j against block_spmv of the device's Z_j: equal values, element by element (the same lane sums the same products in the same
    order in both kernels; alpha = 1, beta = 0 add nothing).
  * Z_1 = d.*R0, Z_{j+1} = d.*AZ_j against numpy's product of the device's own operands: 4 eps |d||w| per element - one complex
    product (with or without contraction of its two terms) against numpy's.
  * H and xi against numpy's Frobenius products OF THE DEVICE'S AZ: n * nrhs * eps of the largest entry - the worst case of a sum of
    that many O(1) products, 1.8e-11 at 5000 x 16; about sqrt(n nrhs) eps is expected.  The measured value is printed.
  * X of one relaxation: 100 * eps * cond(H) of max|X|, cond(H) <= 1e8 asserted on numpy's H (|d| ~ 0.1 for that).
  * ComplexF32: the per-element bounds of tests/test_complex_single_kcycle_gpu.py - the product (m_i + 8) 2^-24 sum |a||z| against
    long double, the directions 3 * 2^-24, the update 4 * 2^-24 (|x0| + sum |t_j||Z_j|) + 100 eps cond(H) max|Z t| with t replayed on
    the host from the device's scalars, rn 1e-10 relative to that replay; H and xi as above (products of widened singles are exact).
  * Cycles: 1e-11 of max|X| against the Kronecker oracle - tests/test_complex_kcycle_gpu.py's bound, measured there with a margin of
    100 at cond(H) up to 6e4.  Every comparison first asserts on the oracle's trace that no rn lies within a factor 4 of 1e-5.
  * ComplexF32 cycles: 4 e_ref, e_ref the distance of the single oracle from the double one on the Kronecker param, computed in the
    same run (the existing rule; it fixes no number).
  * solveMG: the oracle's iteration count, resvec within 1e-10 resvec[0]; block FGMRES: flag 0, the oracle's step count, true
    residual below 1e-8.

64-bit row pointers: the handle's option force_rowptr64 uploads every operator with them, so one relaxation case and one cycle case
run the <long long> instantiations of the new kernels."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import complex_block_fgmres_oracle as bf
import complex_kcycle_block_cases as KB
import complex_kcycle_oracle as korc
import complex_krylov_oracle as ck
import complex_single_kcycle_oracle as sk
from complex_cases import complex_rhs, helmholtz

pytestmark = pytest.mark.gpu

MG_OK, MG_ERR_INVALID, MG_ERR_STATE, MG_ERR_UNSUPPORTED = 0, 1, 3, 4
MG_OP_A = 0
C64, C128 = np.complex64, np.complex128
CLD = np.clongdouble
EPS = np.finfo(float).eps
U32 = 2.0 ** -24
_dp = C.POINTER(C.c_double)
dz = lambda a: a.ctypes.data_as(_dp)
zeros = lambda shape: np.zeros(shape, dtype=C128, order="F")

# ---- one relaxation, piece by piece -----------------------------------------------------------------------------------------------------
_devs = {}


def _relax_dev(mg, name, single=False, wide=False):
    key = (name, single, wide)
    if key not in _devs:
        _devs[key] = mg.device.DeviceHierarchy(KB.relax_param(mg, name, single), options={"force_rowptr64": 1} if wide else None)
    return _devs[key]


@pytest.fixture(scope="module", autouse=True)
def _close_devs():
    yield
    for dev in _devs.values():
        dev.close()
    _devs.clear()


def _check_relaxation(mg, name, nrhs, inner, wide=False):
    p, dev = KB.relax_param(mg, name), _relax_dev(mg, name, wide=wide)
    A, d = p.As[0], p.relaxPrecs[0]
    n = A.shape[0]
    assert n % 256 != 0
    R0, X0 = KB.relax_block(n, nrhs)
    if name == "awkward5000":
        assert A.indptr[2001] - A.indptr[2000] == 3000 and d[2000] != 0 and np.all(R0[2000] != 0)     # the long row feeds every partial
    _, _, Href, _ = KB.relax_bases(A, d, R0, inner)
    cond = np.linalg.cond(Href)
    assert cond <= 1e8
    Xo, rno = KB.relax_oracle(A, d, R0, X0, inner)
    assert len(rno) == inner and min(rno) > 4e-5                  # no break in this case: every direction is used
    X = X0.copy(order="F")
    rn, H, xi, Z, AZ = dev.block_fgmres_relax(1, R0, X, inner, want_bases=True)
    assert Z.shape == AZ.shape == (n, nrhs, inner) and len(rn) == inner
    dcol = d[:, None]
    worst_z = 0.0
    for j in range(inner):
        Zj = np.asfortranarray(Z[:, :, j])
        Y = zeros((n, nrhs))
        dev.block_spmv(1, MG_OP_A, 1.0, Zj, 0.0, Y)
        assert np.array_equal(AZ[:, :, j], Y), f"AZ_{j} differs from block_spmv(Z_{j})"
        src = R0 if j == 0 else AZ[:, :, j - 1]
        zref = dcol * src
        ez, tz = np.abs(Zj - zref), 4 * EPS * np.abs(dcol) * np.abs(src)
        assert np.all(ez[tz == 0] == 0.0)
        worst_z = max(worst_z, float((ez[tz > 0] / tz[tz > 0]).max()))
    Hd, xid = KB.gram_of(AZ, R0)
    eh = np.abs(H - Hd).max() / np.abs(Hd).max()
    ex = np.abs(xi - xid).max() / np.abs(xid).max()
    dx = np.abs(X - Xo).max() / np.abs(Xo).max()
    print(f"{name} nrhs={nrhs} inner={inner} wide={wide}: directions {worst_z:.3f} of 4 eps, H {eh:.2e}  xi {ex:.2e} (bound "
          f"{n * nrhs * EPS:.2e}, sqrt {np.sqrt(n * nrhs) * EPS:.2e})  cond(H) {cond:.2e}  X {dx:.2e} (bound {100 * EPS * cond:.2e})  "
          f"rn {np.abs(rn - rno).max() / max(rno):.2e}")
    assert worst_z <= 1.0
    assert eh <= n * nrhs * EPS and ex <= n * nrhs * EPS
    assert dx <= 100 * EPS * cond
    X2 = X0.copy(order="F")
    rn2, H2, xi2, Z2, AZ2 = dev.block_fgmres_relax(1, R0, X2, inner, want_bases=True)
    for a, b in ((X, X2), (H, H2), (xi, xi2), (rn, rn2), (Z, Z2), (AZ, AZ2)):
        assert a.tobytes() == b.tobytes()
    X3 = X0.copy(order="F")                                       # (without the bases: the same result)
    rn3, H3, _ = dev.block_fgmres_relax(1, R0, X3, inner)
    assert X3.tobytes() == X.tobytes() and H3.tobytes() == H.tobytes() and rn3.tobytes() == rn.tobytes()


@pytest.mark.parametrize("inner", [1, 3, 8])
@pytest.mark.parametrize("nrhs", [1, 3, 4, 16])
@pytest.mark.parametrize("name", ["awkward5000", "oneblock100"])
def test_block_gram_kernel_row_by_row(mg, built, name, nrhs, inner):
    _check_relaxation(mg, name, nrhs, inner)


def test_block_gram_kernel_with_64_bit_row_pointers(mg, built):
    _check_relaxation(mg, "awkward5000", 3, 3, wide=True)


def _ld_product(A, Z):
    """A Z in long double from complex64 data (row sums by reduceat over the non-empty rows), column by column."""
    out = np.zeros(Z.shape, dtype=CLD)
    m = np.diff(A.indptr)
    for c in range(Z.shape[1]):
        prod = A.data.astype(CLD) * Z[:, c].astype(CLD)[A.indices]
        out[m > 0, c] = np.add.reduceat(prod, A.indptr[:-1][m > 0])
    return out


def _replay(H, xi, rnorm0sq, inner, tol=1e-5):
    """The host's loop on the leading blocks of H (complex_kcycle_oracle's algebra): (t, used, rnorms)."""
    rn, t = [], None
    for j in range(inner):
        Hj = H[: j + 1, : j + 1]
        Hj = 0.5 * Hj + 0.5 * Hj.conj().T
        Pinv = korc.julia_pinv(Hj)
        t = korc._cmul(np.ascontiguousarray(Pinv.real), np.ascontiguousarray(Pinv.imag), xi[: j + 1])
        Ht = korc._cmul(np.ascontiguousarray(Hj.real), np.ascontiguousarray(Hj.imag), t)
        rn.append(float(np.sqrt(abs((np.vdot(t, Ht) - 2.0 * np.vdot(t, xi[: j + 1]) + rnorm0sq).real))))
        if rn[-1] < tol:
            break
    return t, len(rn), np.array(rn)


@pytest.mark.parametrize("name,nrhs,inner", [("awkward5000", 3, 3), ("awkward5000", 16, 8), ("awkward5000", 4, 1), ("oneblock100", 1, 8),
                                             ("oneblock100", 16, 3)])
def test_block_relaxation_single_piece_by_piece(mg, built, name, nrhs, inner):
    """A ComplexF32 hierarchy (singleKcycle + blockKcycle): complex128 host blocks holding single values, narrowed on the device."""
    p, dev = KB.relax_param(mg, name, True), _relax_dev(mg, name, True)
    A, d = p.As[0], p.relaxPrecs[0]
    assert A.dtype == C64 and d.dtype == C64
    n = A.shape[0]
    R0, X0 = (np.asfortranarray(a.astype(C64).astype(C128)) for a in KB.relax_block(n, nrhs))
    X = X0.copy(order="F")
    rn, H, xi, Z, AZ = dev.block_fgmres_relax(1, R0, X, inner, want_bases=True)
    assert len(rn) == inner
    for a in (X, Z, AZ):                                          # widened singles, exactly
        assert np.array_equal(a.astype(C64).astype(C128), a)
    absA = sp.csr_matrix((np.abs(A.data.astype(C128)), A.indices, A.indptr), shape=A.shape)
    dcol = d.astype(C128)[:, None]
    worst_w = worst_z = 0.0
    for j in range(inner):
        Zj = Z[:, :, j]
        err = np.abs(AZ[:, :, j].astype(CLD) - _ld_product(A, Zj.astype(C64))).astype(np.float64)
        bound = (np.diff(A.indptr) + 8)[:, None] * U32 * (absA @ np.abs(Zj))
        nz = bound > 0
        assert np.all(err[~nz] == 0.0)                            # empty rows: exact zeros
        worst_w = max(worst_w, float((err[nz] / bound[nz]).max()))
        zref = dcol * (R0 if j == 0 else AZ[:, :, j - 1])
        ez, tz = np.abs(Zj - zref), 3 * U32 * np.abs(zref)
        assert np.all(ez[tz == 0] == 0.0)
        worst_z = max(worst_z, float((ez[tz > 0] / tz[tz > 0]).max()))
    W = AZ.reshape(-1, inner).astype(CLD)
    Href = (W.conj().T @ W).astype(C128)
    xiref = (W.conj().T @ R0.reshape(-1).astype(CLD)).astype(C128)
    eh = np.abs(H - Href).max() / np.abs(Href).max()
    ex = np.abs(xi - xiref).max() / np.abs(xiref).max()
    cond = np.linalg.cond(Href)
    assert cond <= 1e8
    r0l = R0.reshape(-1).astype(CLD)
    t, used, rnref = _replay(H, xi, float((r0l.real ** 2 + r0l.imag ** 2).sum()), inner)
    assert used == inner and min(rnref) > 4e-5
    Zt = Z @ t
    bound_x = 4 * U32 * (np.abs(X0) + np.abs(Z) @ np.abs(t)) + 100 * EPS * cond * np.abs(Zt).max()
    wx = float((np.abs(X - (X0 + Zt)) / bound_x).max())
    er = (np.abs(rn - rnref) / rnref).max()
    print(f"CF32 {name} nrhs={nrhs} inner={inner}: product {worst_w:.3f} of its row bound, directions {worst_z:.3f} of 3*2^-24, "
          f"H {eh:.2e}, xi {ex:.2e} (bound {n * nrhs * EPS:.2e}), cond(H) {cond:.2e}, X {wx:.3f} of its bound, rn {er:.2e}")
    assert worst_w <= 1.0 and worst_z <= 1.0
    assert eh <= n * nrhs * EPS and ex <= n * nrhs * EPS
    assert wx <= 1.0 and er <= 1e-10
    X2 = X0.copy(order="F")
    rn2, H2, xi2, Z2, AZ2 = dev.block_fgmres_relax(1, R0, X2, inner, want_bases=True)
    for a, b in ((X, X2), (H, H2), (xi, xi2), (rn, rn2), (Z, Z2), (AZ, AZ2)):
        assert a.tobytes() == b.tobytes()


def test_block_relaxation_breaks_after_the_first_direction(mg, built):
    p, dev = KB.relax_param(mg, "awkward5000"), _relax_dev(mg, "awkward5000")
    A, d = p.As[0], p.relaxPrecs[0]
    R0, _ = KB.relax_block(A.shape[0], 3, scale=1e-9)
    X0 = np.zeros_like(R0)                                        # (the update is ~1e-10: it would drown in an X of O(1))
    Xo, rno = KB.relax_oracle(A, d, R0, X0, 3)
    assert len(rno) == 1 and rno[0] < 1e-5 / 4                    # on the oracle alone
    X = X0.copy(order="F")
    rn, H, xi = dev.block_fgmres_relax(1, R0, X, 3)
    assert len(rn) == 1                                           # used == 1
    assert abs(rn[0] - rno[0]) <= 1e-10 * rno[0]
    assert np.abs(X - Xo).max() <= 1e-11 * np.abs(Xo).max()
    assert H[2, 2].real > 0                                       # the directions behind the break were summed all the same


def test_the_columns_are_coupled_as_in_the_oracle(mg, built):
    """Two columns, one scaled by 1e3: the device equals the long-vector oracle and differs from two vector relaxations."""
    p, dev = KB.relax_param(mg, "awkward5000"), _relax_dev(mg, "awkward5000")
    A, d = p.As[0], p.relaxPrecs[0]
    R0, X0 = KB.relax_block(A.shape[0], 2)
    R0[:, 1] *= 1e3
    Xo, rno = KB.relax_oracle(A, d, R0, X0, 3)
    assert len(rno) == 3 and min(rno) > 4e-5
    X = X0.copy(order="F")
    dev.block_fgmres_relax(1, R0, X, 3)
    Xv = X0.copy(order="F")
    for c in range(2):
        col = np.ascontiguousarray(Xv[:, c])
        dev.fgmres_relax(1, np.ascontiguousarray(R0[:, c]), col, 3)
        Xv[:, c] = col
    e_blk = np.abs(X - Xo).max() / np.abs(Xo).max()
    e_col = np.abs(X - Xv).max() / np.abs(Xo).max()
    print(f"coupling: device block against the block oracle {e_blk:.2e}, against two vector relaxations {e_col:.2e}")
    assert e_blk <= 1e-11
    assert e_col > 1e-6


# ---- cycles against the Kronecker oracle ------------------------------------------------------------------------------------------------
CYCLE_CASES = [(prob, s, k) for prob in ("3lev", "4lev") for s in KB.SCHEDULES for k in KB.KS]


def _device_two_cycles(mg, p, B, sparse=False, options=None):
    dev = mg.device.DeviceHierarchy(p, options=options)
    try:
        if sparse:                                                # the coarsest solve from the complex sparse factors
            dev._set_coarse(p, force_sparse=True)
            assert dev.lib.mg_finalize(dev.handle) == 0
        X = zeros(B.shape)
        dev.block_cycle(B, X, 1)
        X1 = X.copy(order="F")
        dev.block_cycle(B, X, -1)
        return X1, X
    finally:
        dev.close()


def _compare_two_cycles(mg, tag, ref, **kw):
    X1, X2 = _device_two_cycles(mg, ref["p"], ref["B"], **kw)
    e1 = np.abs(X1 - ref["X1"]).max() / np.abs(ref["X1"]).max()
    e2 = np.abs(X2 - ref["X2"]).max() / np.abs(ref["X2"]).max()
    print(f"{tag}: cycle 1 {e1:.2e}, cycle 2 {e2:.2e}")
    assert e1 <= 1e-11 and e2 <= 1e-11


@pytest.mark.parametrize("prob,sched,k", CYCLE_CASES, ids=KB.case_id)
def test_two_block_cycles_against_the_oracle(mg, built, prob, sched, k):
    ref = KB.two_cycles(mg, prob, sched, k, 1.0)
    assert len(ref["trace"]) > 0 and korc.rn_clear_of_tol(ref["trace"], 4.0), korc.all_rn(ref["trace"])      # on the oracle alone
    _compare_two_cycles(mg, f"{prob} {sched} k={k}", ref)


@pytest.mark.parametrize("prob,sched,k", CYCLE_CASES, ids=KB.case_id)
def test_two_block_cycles_with_the_break(mg, built, prob, sched, k):
    """The block scaled by 1e-11: the oracle breaks after the first direction in every relaxation."""
    ref = KB.two_cycles(mg, prob, sched, k, KB.BREAK_SCALE)
    assert len(ref["trace"]) > 0 and korc.rn_clear_of_tol(ref["trace"], 4.0)
    assert all(rec[3] == 1 for rec in ref["trace"])
    _compare_two_cycles(mg, f"{prob} {sched} k={k} (break)", ref)


def test_two_block_cycles_with_sparse_coarsest_factors(mg, built):
    ref = KB.two_cycles(mg, "4lev", ("Jac-GMRES", "K", 2, 1), 3, 1.0)
    assert korc.rn_clear_of_tol(ref["trace"], 4.0)
    _compare_two_cycles(mg, "4lev Jac-GMRES K(2,1) k=3, sparse factors", ref, sparse=True)


def test_two_block_cycles_with_64_bit_row_pointers(mg, built):
    ref = KB.two_cycles(mg, "4lev", ("Jac-GMRES", "K", 2, 1), 3, 1.0)
    assert korc.rn_clear_of_tol(ref["trace"], 4.0)
    _compare_two_cycles(mg, "4lev Jac-GMRES K(2,1) k=3, 64-bit row pointers", ref, options={"force_rowptr64": 1})


def test_block_cycle_with_the_gmres_coarsest_solve(mg, built):
    """coarseSolveType="GMRES" with blockCoarseGMRES and blockKcycle: the block coarsest solve inside the block K-cycle."""
    import complex_block_coarse_cases as cbc
    ref = KB.gmres_coarse_cycle(mg)
    assert len(ref["trace"]) > 0 and korc.rn_clear_of_tol(ref["trace"], 4.0)
    assert len(ref["log"]) > 0 and cbc.clearance(ref["log"]) >= cbc.MIN_CLEARANCE, cbc.clearance(ref["log"])
    dev = mg.device.DeviceHierarchy(ref["p"])
    try:
        X = zeros(ref["B"].shape)
        dev.block_cycle(ref["B"], X, 1)
    finally:
        dev.close()
    err = np.abs(X - ref["X1"]).max() / np.abs(ref["X1"]).max()
    print(f"GMRES coarsest solve under a block K-cycle: {err:.2e} (coarse clearance {cbc.clearance(ref['log']):.2f})")
    assert err <= 1e-11                                           # (the cycles' bound; tests/test_complex_block_coarse_gmres_gpu.py's too)
    q = KB.helm_param(mg, KB.GMRES_COARSE[0], KB.GMRES_COARSE[1], damping=KB.GMRES_COARSE[2], coarse="GMRES")     # no blockCoarseGMRES
    with pytest.raises(NotImplementedError):
        mg.recursiveCycle(q, ref["B"], zeros(ref["B"].shape))
    mg.clear_(q)


# ---- ComplexF32 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob,sched,k", [("3lev", ("Jac-GMRES", "V", 2, 2), 3), ("4lev", ("Jac-GMRES", "K", 2, 1), 3), ("4lev", ("Jac", "K", 2, 1), 16)],
                         ids=KB.case_id)
def test_single_block_cycle_through_the_mixed_closure(mg, built, prob, sched, k):
    p = KB.helm_param(mg, prob, sched, singlePrecision=True, singleKcycle=True)
    try:
        B = KB.block_rhs(p.As[0].shape[0], k)
        q = KB.kron_param(p, k)
        t64, ts = [], []
        bl = KB.flat(B).astype(C64)
        x64 = korc.recursiveCycle(sk.rounded(q), bl.astype(C128), np.zeros(bl.shape, dtype=C128), 1, trace=t64).copy()
        xs = sk.recursiveCycle(q, bl, np.zeros_like(bl), 1, trace=ts).copy()
        used = lambda tr: [(r[0], r[1], r[2], r[3]) for r in tr]
        assert len(ts) > 0 and used(ts) == used(t64)                                           # the inputs' properties, on the oracles
        assert korc.rn_clear_of_tol(ts, 4.0) and korc.rn_clear_of_tol(t64, 4.0)
        e_ref = float(np.abs(xs.astype(C128) - x64).max() / np.abs(x64).max())
        assert e_ref <= 1e-3
        M = mg.getMultigridPreconditioner(p, B)
        Xd = np.array(M(B))
        e_dev = float(np.abs(KB.flat(Xd) - x64).max() / np.abs(x64).max())
        print(f"CF32 {prob} {sched} k={k}: e_ref {e_ref:.3e}, device {e_dev:.3e} ({e_dev / e_ref:.2f} e_ref)")
        assert e_dev <= 4 * e_ref
    finally:
        mg.clear_(p)


# ---- the public surfaces ----------------------------------------------------------------------------------------------------------------
def test_solveMG_on_a_block(mg, built):
    """Five iterations from X = 0 on 3 columns.  The block is scaled by 1e5, as tests/test_complex_kcycle_gpu.py's _solve_case scales
    its vector, so that every rn of the five cycles stays two decades or more above the break (asserted on the oracle)."""
    p = KB.helm_param(mg, "4lev", ("Jac-GMRES", "K", 2, 1))
    try:
        k = 3
        B = KB.block_rhs(p.As[0].shape[0], k, 1e5)
        trace, hist = [], {}
        xo, ito = korc.solveMG(KB.kron_param(p, k), KB.flat(B), np.zeros(B.size, dtype=C128), hist, trace)
        rn = korc.all_rn(trace)
        assert rn.size > 0 and rn.min() >= 100 * 1e-5, rn.min()
        X = zeros(B.shape)
        _, _, it = mg.solveMG(p, B, X)
        dr = np.abs(p.resvec - hist["resvec"]).max() / hist["resvec"][0]
        dx = np.abs(KB.flat(X) - xo).max() / np.abs(xo).max()
        print(f"block solveMG: {it} ({ito}) iterations, resvec diff {dr:.2e}, X diff {dx:.2e}, relres {hist['resvec'][-1] / hist['resvec'][0]:.2e}")
        assert it == ito == 5 and len(p.resvec) == len(hist["resvec"])
        assert dr <= 1e-10 and dx <= 1e-10
        X2 = zeros(B.shape)                                       # recursiveCycle on the 2-D array: the first iterate of that solve
        mg.recursiveCycle(p, B, X2)
        ref1 = korc.recursiveCycle(KB.kron_param(p, k), KB.flat(B), np.zeros(B.size, dtype=C128), 1)
        assert np.abs(KB.flat(X2) - ref1).max() <= 1e-11 * np.abs(ref1).max()
    finally:
        mg.clear_(p)


def test_block_fgmres_with_a_block_kcycle_preconditioner(mg, built):
    """solveBlockGMRES_MG_CFP64 with a K(2,1) Jac hierarchy (damping 0.5) on the less damped system operator (0.05), k = 3, against
    tests/complex_block_fgmres_oracle.py with the Kronecker oracle as M."""
    cells, kh, _ = KB.PROBLEMS["4lev"]
    As, _ = helmholtz(mg, cells, kh, 0.05)
    p = KB.helm_param(mg, "4lev", ("Jac", "K", 2, 1), maxIter=ck.MAXIT_FGMRES, tol=ck.TOL)
    try:
        k = 3
        B = KB.block_rhs(As.shape[0], k, 1e6)
        trace = []
        Xo, fo, ito, rvo = bf.blockFGMRES(lambda V: As @ V, B, 5, ck.TOL, ck.MAXIT_FGMRES, KB.kron_preconditioner(p, k, trace))
        assert fo == 0 and korc.rn_clear_of_tol(trace, 4.0), korc.all_rn(trace).min()
        X = zeros(B.shape)
        _, _, it, rv = mg.solveBlockGMRES_MG_CFP64(As, p, B, X, True, 5)
        res = np.linalg.norm(B - As @ X) / np.linalg.norm(B)
        print(f"block FGMRES(5) with K(2,1) Jac: flag {p.flag}, {it} ({ito}) steps, true residual {res:.3e}, "
              f"X diff {np.abs(X - Xo).max() / np.abs(Xo).max():.2e}")
        assert p.flag == 0 and it == ito and len(rv) == len(rvo)
        assert res < 1e-8
        # block BiCGSTAB and the solver object run on the same hierarchy (a linear cycle: K with Jac)
        import complex_block_oracle as cb
        trace = []
        _, fb, itb, _ = cb.blockBiCGSTB(lambda V: As @ V, B, ck.TOL, ck.MAXIT_BICGSTAB, KB.kron_preconditioner(p, k, trace))
        assert fb in (0, -3) and korc.rn_clear_of_tol(trace, 4.0), korc.all_rn(trace).min()
        p.maxOuterIter = ck.MAXIT_BICGSTAB
        X = zeros(B.shape)
        _, _, it, _ = mg.solveBlockBiCGSTAB_MG_CFP64(As, p, B, X)
        res = np.linalg.norm(B - As @ X) / np.linalg.norm(B)
        print(f"block BiCGSTAB with K(2,1) Jac: flag {p.flag} ({fb}), {it} ({itb}) iterations, true residual {res:.3e}")
        assert (p.flag, it) == (fb, itb) and res < 1e-8
    finally:
        mg.clear_(p)


def test_replace_matrix_then_a_block_cycle(mg, built):
    """K with SPAI stays in HBM (the vector rule); the block cycle behind it equals the oracle on a fresh hierarchy."""
    p = KB.helm_param(mg, "4lev", ("SPAI", "K", 2, 1))
    fresh = KB.helm_param(mg, "4lev", ("SPAI", "K", 2, 1), damping=0.3)
    try:
        k = 3
        B = KB.block_rhs(p.As[0].shape[0], k)
        mg.recursiveCycle(p, B, zeros(B.shape))                   # uploads
        dev = p.device
        assert dev is not None
        cells, kh, _ = KB.PROBLEMS["4lev"]
        A2, _ = helmholtz(mg, cells, kh, 0.3)
        mg.replaceMatrixInHierarchy(p, A2)
        assert p.device is dev                                    # refreshed in HBM, not uploaded again
        trace = []
        xo = korc.recursiveCycle(KB.kron_param(fresh, k), KB.flat(B), np.zeros(B.size, dtype=C128), 1, trace=trace)
        assert korc.rn_clear_of_tol(trace, 4.0), korc.all_rn(trace)
        X = zeros(B.shape)
        mg.recursiveCycle(p, B, X)
        err = np.abs(KB.flat(X) - xo).max() / np.abs(xo).max()
        print(f"block cycle after replaceMatrixInHierarchy: {err:.2e}")
        assert err <= 1e-11
    finally:
        mg.clear_(p)
        mg.clear_(fresh)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_without_the_flag_every_block_entry_is_refused_as_before(mg, built):
    lib = mg.device.load_library()
    p = KB.helm_param(mg, "3lev", ("Jac-GMRES", "K", 2, 1), blockKcycle=False)
    n = p.As[0].shape[0]
    B, X = KB.block_rhs(n, 2), zeros((n, 2))
    dev = mg.device.DeviceHierarchy(p)
    try:
        hc = dev.handle
        lz = C.c_longlong(0)
        lp = C.byref(lz)
        res, ab, H = np.zeros(64), np.array([1.0, 0.0]), np.zeros(2 * 81)
        msg = b"blocks of right-hand sides are not served on a K-cycle / Jac-GMRES complex hierarchy"

        def refused(rc, code=MG_ERR_UNSUPPORTED, text=msg):
            assert rc == code, (rc, lib.mg_last_error())
            assert text in lib.mg_last_error(), lib.mg_last_error()

        refused(lib.mg_block_cycle_CF64(hc, dz(B), dz(X), n, 2, 1))
        refused(lib.mg_block_solve_CF64(hc, dz(B), dz(X), n, 2, 1e-6, 2, lp, dz(res)))
        refused(lib.mg_block_spmv_CF64(hc, 1, 0, dz(ab), dz(B), dz(ab), dz(X), 2))
        refused(lib.mg_block_bicgstab_CFP64(hc, dz(B), dz(X), n, 2, 1e-6, 2, lp, lp, dz(res), lp))
        refused(lib.mg_block_fgmres_CFP64(hc, dz(B), dz(X), n, 2, 5, 1e-6, 2, lp, lp, dz(res), lp))
        refused(lib.mg_block_fgmres_relax_CF64(hc, 1, dz(B), dz(X), n, 2, 2, 1e-5, dz(H), dz(H), dz(H), lp, None, None),
                text=b"without the option kcycle_blocks")
        assert not X.any()
        for call in (lambda: dev.block_cycle(B, X, 1), lambda: dev.block_solve(B, X, 1e-6, 2), lambda: dev.block_bicgstab(B, X, 1e-6, 2),
                     lambda: dev.block_fgmres(B, X, 5, 1e-6, 2), lambda: dev.block_fgmres_relax(1, B, X, 2)):
            with pytest.raises(NotImplementedError, match="K-cycle / Jac-GMRES"):
                call()
        x = np.zeros(n, dtype=C128)                               # the handle still serves a vector
        dev.cycle(np.ascontiguousarray(B[:, 0]), x, 1)
        assert np.isfinite(x).all() and x.any()
    finally:
        dev.close()
    for call in (lambda: mg.solveMG(p, B, X), lambda: mg.recursiveCycle(p, B, X), lambda: mg.getMultigridPreconditioner(p, B)(B)):
        with pytest.raises(NotImplementedError):
            call()
    mg.clear_(p)


def test_refusals_with_the_flag_leave_the_handle_usable(mg, built):
    lib = mg.device.load_library()
    ref = KB.two_cycles(mg, "3lev", ("Jac-GMRES", "K", 2, 1), 3, 1.0)
    assert korc.rn_clear_of_tol(ref["trace"], 4.0)
    p, B = ref["p"], ref["B"]
    n = B.shape[0]
    dev = mg.device.DeviceHierarchy(p)
    A8, mesh8 = mg.poisson_shifted([8, 8, 8])
    pr = mg.getMGparam(np.float64, np.int64, 2, 8, 4, 1e-10, "Jac", 0.8, 1, 1, "V")
    mg.MGsetup(A8, mesh8, pr)
    rdev = mg.device.DeviceHierarchy(pr)
    try:
        hc = dev.handle
        lz = C.c_longlong(0)
        lp = C.byref(lz)
        H = np.zeros(2 * 81)

        def refused(rc, code):
            assert rc == code, (rc, lib.mg_last_error())
            assert lib.mg_last_error()

        B17, X17 = zeros((n, 17)), zeros((n, 17))
        B17[...] = 1.0
        refused(lib.mg_block_cycle_CF64(hc, dz(B17), dz(X17), n, 17, 1), MG_ERR_UNSUPPORTED)                 # 17 columns
        assert b"at most 16" in lib.mg_last_error()
        relax = lambda nrhs, inner, Z=None: lib.mg_block_fgmres_relax_CF64(hc, 1, dz(B17), dz(X17), n, nrhs, inner, 1e-5, dz(H), dz(H),
                                                                           dz(H), lp, Z, Z)
        refused(relax(17, 2), MG_ERR_UNSUPPORTED)
        refused(relax(0, 2), MG_ERR_INVALID)
        refused(relax(2, 9), MG_ERR_UNSUPPORTED)                                                             # 9 directions
        refused(relax(2, 0), MG_ERR_INVALID)
        refused(lib.mg_block_fgmres_relax_CF64(hc, 3, dz(B17), dz(X17), n, 2, 2, 1e-5, dz(H), dz(H), dz(H), lp, None, None), MG_ERR_INVALID)
        refused(lib.mg_block_fgmres_relax_CF32(hc, 1, dz(B17), dz(X17), n, 2, 2, 1e-5, dz(H), dz(H), dz(H), lp, None, None), MG_ERR_STATE)
        assert not X17.any()
        refused(lib.mg_block_fgmres_relax_CF64(rdev.handle, 1, dz(B17), dz(X17), n, 2, 2, 1e-5, dz(H), dz(H), dz(H), lp, None, None),
                MG_ERR_STATE)                                                                                # a real handle
        assert lib.mg_set_option(rdev.handle, b"kcycle_blocks", 1.0) == MG_OK                                # (an option of every handle:
        refused(lib.mg_block_cycle_CF64(rdev.handle, dz(B17), dz(X17), A8.shape[0], 2, 1), MG_ERR_STATE)     #  a real one stays refused)
        refused(lib.mg_set_cycle_type(hc, ord("K")), MG_ERR_UNSUPPORTED)                                     # the shared setters
        refused(lib.mg_set_relax_type(hc, 1), MG_ERR_UNSUPPORTED)
        with pytest.raises(NotImplementedError):
            mg.getMGparam(np.float64, np.int64, 2, 8, 4, 1e-10, "Jac", 0.8, 1, 1, "K", blockKcycle=True)
        # relaxPre = 9 with Jac-GMRES still fails at mg_finalize; then the handle is set right again
        d1 = np.ascontiguousarray(p.relaxPrecs[0], dtype=C128)
        assert lib.mg_set_relax_CF64(hc, 1, dz(d1), n, 9, 1) == MG_OK
        refused(lib.mg_finalize(hc), MG_ERR_UNSUPPORTED)
        refused(lib.mg_block_cycle_CF64(hc, dz(B17), dz(X17), n, 2, 1), MG_ERR_STATE)
        assert lib.mg_set_relax_CF64(hc, 1, dz(d1), n, 2, 1) == MG_OK
        assert lib.mg_finalize(hc) == MG_OK
        # the option read at every call: switched off it refuses, switched on again the handle runs the oracle's cycle
        assert lib.mg_set_option(hc, b"kcycle_blocks", 0.0) == MG_OK
        X = zeros(B.shape)
        refused(lib.mg_block_cycle_CF64(hc, dz(B), dz(X), n, 3, 1), MG_ERR_UNSUPPORTED)
        assert lib.mg_set_option(hc, b"kcycle_blocks", 1.0) == MG_OK
        dev.block_cycle(B, X, 1)
        assert np.abs(X - ref["X1"]).max() <= 1e-11 * np.abs(ref["X1"]).max()
        x = np.zeros(n, dtype=C128)                               # and the vector form next to it is the vector oracle's
        b0 = np.ascontiguousarray(B[:, 0])
        dev.cycle(b0, x, 1)
        xo = korc.recursiveCycle(p, b0, np.zeros_like(b0), 1)
        assert np.abs(x - xo).max() <= 1e-11 * np.abs(xo).max()
    finally:
        dev.close()
        rdev.close()
    # a Schwarz coarsest solve on a block: MG_ERR_UNSUPPORTED with its present message, and the vector form still runs
    import coarse_solver_cases as csc
    A2, mesh2 = helmholtz(mg, [32, 32], 0.5, 0.5)
    ps = csc.setup(mg, A2, mesh2, 3, csc.dd_lu(mg, mesh2, [2, 2], [1, 1], np.complex128), np.complex128, "Jac", 0.8, 2, 1, "K", 12, 1e-8)
    ps.blockKcycle = True
    sdev = mg.device.DeviceHierarchy(ps)
    try:
        Bs = KB.block_rhs(A2.shape[0], 2)
        with pytest.raises(mg.device.MGDeviceError, match=rf"status {MG_ERR_UNSUPPORTED}\b.*Schwarz"):
            sdev.block_cycle(Bs, zeros(Bs.shape), 1)
        xs = np.zeros(A2.shape[0], dtype=C128)
        sdev.cycle(np.ascontiguousarray(Bs[:, 0]), xs, 1)
        assert np.isfinite(xs).all() and xs.any()
    finally:
        sdev.close()
        mg.clear_(ps)
    # Vanka with 'K' on a block: refused by the Python layer before the device is touched
    import complex_vanka_cases as vcase
    name = next(iter(vcase.CASES))
    nv, levels, omega, _ = vcase.CASES[name]
    pv = mg.getMGparam(np.complex128, np.int64, levels, 1, 5, 1e-30, "VankaFaces", vcase.W, 1, 1, "K", "NoMUMPS", 0.4, 0.0,
                       "SystemsFacesMixedLinear", complexVanka=True, vankaBlocks=True, blockKcycle=True)
    mg.MGsetup(vcase.operator(nv, omega), vcase.mesh(mg, nv), pv)
    Bv = zeros((pv.As[0].shape[0], 2))
    Bv[...] = 1.0
    with pytest.raises(NotImplementedError, match="K-cycle complex Vanka"):
        mg.recursiveCycle(pv, Bv, zeros(Bv.shape))
    mg.clear_(pv)
