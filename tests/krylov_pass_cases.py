"""TEST INFRASTRUCTURE ONLY.  Shapes, seeded inputs, long-double references, bounds and plain fp64 restatements for the passes of the
real single-GPU Krylov drivers (pcg_dev, bicgstab_dev, FgmresCore and the block drivers of csrc/mg_krylov.inc; kernels in
csrc/mg_kernels.hpp), taken one by one through mg_kry_*_dev_FP64 and mg_vec_dscale / xpdr / sumsq_dev_FP64
(tests/test_krylov_passes_host.py, tests/test_krylov_passes_gpu.py).  numpy only: imports no device code of the package.

Every `check_*` takes what a pass produced (from the device, or from a restatement below) with the inputs it was given, compares it
with numpy long double of the same expression and returns the worst ratio of error to bound (asserting it is at most 1).  NaN fails.

Bounds (derived; never measured from a device).  u = 2^-53.
  vector   an updated element is within 2 ulp of the largest magnitude among its expression's terms, partial results and result
           (krylov_bounds._close_vec: every rounding of the unfused evaluation is at most half an ulp of one of them, at most four).
  sum      |got - sum| <= n u sum|terms| for n terms (krylov_bounds._close_sum: any order of summation of fp64 products).
  norm     the drivers return sqrt(s) of the device's sum s, the root taken on the host: got = sqrt(s)(1 + d), |d| <= u, so
           got^2 = s (1 + d)^2 and |got^2 - S| <= |s - S| + (2u + u^2) s <= (n + 3) u S for the long-double S = sum x_i^2 (all terms
           positive, s <= S (1 + n u)); got^2 is formed in long double (2^-64, inside the third unit).
  Gram     every entry is a sum of n products: the sum bound with n terms.
  blk_comb the kernel forms o = s * add first (one rounding; 0 without add), then o += in[i, a] * C[a, b] for a = 0 .. k-1 in that order.
           A term passes through its own product (no rounding when the compiler fuses it) and at most k additions: at most k + 1
           roundings, (1 + u)^(k+1) - 1 <= (k + 1) u + O(k^2 u^2); one more unit covers the second-order terms (k <= 16: k^2 u < 1e-13).
           |got - ref| <= (k + 2) u (|s add| + sum_a |in_ia| |C_ab|).  The kernel MULTIPLIES s and add (mg_kernels.hpp: `s * add[...]` whenever
           add is given): with s == 0 a NaN of add reaches the result in exactly its own entry, and nowhere without add.
"""
import numpy as np

from krylov_bounds import LD, U, _close_sum, _close_vec, _ld

assert np.finfo(LD).nmant >= 63, "the references need a 64-bit significand"

# ---- the launch geometry of the kernels (mg_kernels.hpp, mg_launch.inc, mg_schedule.inc, mg_krylov.inc) ------------------------------
BLK = 256            # MG_BLK: threads per workgroup
NRED_BLOCKS = 1024   # mg_hierarchy::nred_blocks: the reductions (dot_partial, sumsq_partial, mgs_step) launch at most this many
#                      workgroups, one 16-byte PAIR per lane and trip: NRED_BLOCKS * BLK pairs per trip
GRID_CAP = 2048      # grid_for(): the element-wise kernels launch at most this many workgroups, one ELEMENT per lane and trip
GRAM_CAP = 256       # blk_gram: at most this many workgroups, one ROW per lane and trip
KMAX = 16            # BLK_KMAX
# Both caps of the vector kernels end at the same length: 2 * NRED_BLOCKS * BLK == GRID_CAP * BLK == 524 288 elements.  One element
# more and grid_for's kernels wrap into their grid-stride loop (lane 0 of workgroup 0 takes element 524 288 on a second trip), while the
# reductions run their capped grid completely full - every lane of all 1024 workgroups holds exactly one pair - and the odd tail goes
# to lane 0 of workgroup 0 on top.  The reductions' own second trip (pair 262 144, at 524 290 elements) is inside 1 000 003.
CAP_N = GRID_CAP * BLK + 1
assert CAP_N == 2 * NRED_BLOCKS * BLK + 1 == 524_289
VEC_N = (1, 2, 3, 511, 512, 513, CAP_N, 1_000_003)
# blk_gram wraps beyond GRAM_CAP * BLK = 65 536 rows
BLK_N = (1, 255, 256, 257, 70_001)
assert BLK_N[-1] > GRAM_CAP * BLK
BLK_K = (1, 2, 3, 5, 8, 16)
LAYOUTS = (0, 1, 2)          # every vector on a 16-byte boundary; every vector 8 bytes past one; mixed (every other one)
NRHS = (1, 2, 3, 4, 16)      # mg_vec_dscale / xpdr: the pair path, the even-nrhs pair path (on a boundary; off it: the element path), the element path
CHAIN_I = (0, 1, 7)          # at every vector n; and the last slot of the 66-double readback:
CHAIN_LAST = (513, 63)

GUARD = 64                               # doubles on each side of a view (512 bytes: the view keeps its alignment class)
SENTINEL = np.int64(0x7FF4DEADBEEF5A5A)  # a signalling-NaN bit pattern: no kernel writes it (tests/default_paths_check.py)

ALPHA, BETA = 0.37, -1.3


def offset(layout, c):
    """Doubles past a 16-byte boundary of the c-th vector of a case."""
    return 1 if (layout == 1 or (layout == 2 and c % 2 == 1)) else 0


def vectors(n, count, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n) for _ in range(count)]


def block(n, k, seed):
    return np.random.default_rng(seed).standard_normal((n, k))


def coeff(k, seed):
    """A dense k x k coefficient matrix without symmetry: C[a, b] != C[b, a] for every a != b, so a transposed index shows."""
    Cm = np.random.default_rng(seed).uniform(0.5, 1.5, (k, k))
    Cm[np.tril_indices(k, -1)] *= -1.0
    return Cm


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- checks: what a pass produced against long double -----------------------------------------------------------------------------------
def check_dot(name, got, x, y):
    return _close_sum(name, got, _ld(x) * _ld(y))


def check_sumsq(name, got, x):
    return _close_sum(name, got, _ld(x) * _ld(x))


def check_norm(name, got, x):
    """(n + 3) u S on the square (module docstring)."""
    t = _ld(x) * _ld(x)
    S, bound = t.sum(), (t.size + 3) * LD(U) * t.sum()
    err = abs(LD(got) * LD(got) - S)
    print(f"    {name}: |norm^2 - reference| = {float(err):.3e} (bound {float(bound):.3e})")
    assert err <= bound and got >= 0.0, (name, float(err), float(bound))
    return float(err / bound) if bound > 0 else 0.0


def check_axpby(name, got, a, x, b, y):
    """y = a x + b y; b == 0: a x alone (y is not read: whatever it held, NaN included, stays out)."""
    ax = LD(a) * _ld(x)
    if b == 0.0:
        return _close_vec(name, got, ax)
    by = LD(b) * _ld(y)
    return _close_vec(name, got, ax + by, ax, by)


def check_cg_update(name, got_x, got_r, alpha, p, Ap, x0, r0, got_norm=None):
    ap, aq = LD(alpha) * _ld(p), LD(alpha) * _ld(Ap)
    worst = max(_close_vec(name + " x", got_x, _ld(x0) + ap, _ld(x0), ap), _close_vec(name + " r", got_r, _ld(r0) - aq, _ld(r0), aq))
    if got_norm is not None:                       # the norm of the r the pass itself produced
        worst = max(worst, check_norm(name + " ||r||", got_norm, got_r))
    return worst


def check_cg_p(name, got, beta, z, p0):
    bp = LD(beta) * _ld(p0)
    return _close_vec(name, got, _ld(z) + bp, _ld(z), bp)


def check_mgs_step(name, got_w, got_out, hk, v, w0, u):
    """w = w0 - hk v within the vector bound; out = w'u (u None: w'w) of the w the pass itself produced, within the sum bound."""
    hv = LD(hk) * _ld(v)
    worst = _close_vec(name + " w", got_w, _ld(w0) - hv, _ld(w0), hv)
    other = got_w if u is None else u
    return max(worst, _close_sum(name + " sum", got_out, _ld(got_w) * _ld(other)))


def check_dscale(name, got, d, b):
    """x[i, c] = d[i] b[i, c] (b, got: [n, nrhs])."""
    return _close_vec(name, got, _ld(d)[:, None] * _ld(b))


def check_xpdr(name, got, x, d, r):
    dr = _ld(d)[:, None] * _ld(r)
    return _close_vec(name, got, _ld(x) + dr, _ld(x), dr)


def check_gram(name, G, X, Y):
    """G[a, b] = sum_i X[i, a] Y[i, b]: the sum bound with n terms, entry by entry."""
    Xl, Yl = _ld(X), _ld(Y)
    n, k = Xl.shape
    assert G.shape == (k, k)
    worst = 0.0
    for a in range(k):
        t = Xl[:, a:a + 1] * Yl                                 # [n, k]: the terms of row a of G
        ref, bound = t.sum(axis=0), n * LD(U) * np.abs(t).sum(axis=0)
        err = np.abs(_ld(G[a]) - ref)
        assert np.all(err <= bound), (name, a, err.astype(float), bound.astype(float))
        worst = max(worst, float((err / np.where(bound > 0, bound, 1)).max()))
    print(f"    {name}: worst entry at {worst:.3f} of its bound")
    return worst


def check_comb(name, got, add, s, inp, Cm):
    """out = s add + inp Cm within (k + 2) u (|s add| + |inp| |Cm|); a NaN of add comes back in exactly its own entry."""
    il, Cl = _ld(inp), _ld(Cm)
    k = Cl.shape[0]
    if add is None:
        sa, nan = np.zeros_like(il), np.zeros(il.shape, dtype=bool)
    else:
        nan = np.isnan(add)
        sa = LD(s) * np.where(nan, LD(0), _ld(add))
    ref = sa + il @ Cl
    bound = (k + 2) * LD(U) * (np.abs(sa) + np.abs(il) @ np.abs(Cl))
    gn = np.isnan(got)
    assert np.array_equal(gn, nan), (name, "NaN entries", int(gn.sum()), int(nan.sum()))
    err = np.where(nan, LD(0), np.abs(_ld(np.where(gn, 0.0, got)) - ref))
    ratio = err / np.where(bound > 0, bound, 1)
    worst = float(ratio.max())
    print(f"    {name}: worst entry at {worst:.3f} of its bound")
    assert np.all(err <= bound), (name, worst)
    return worst


# ---- crafted inputs -------------------------------------------------------------------------------------------------------------------------
def chain_breakdown(n, i):
    """V_0 = e_1, V_1 .. V_i = e_2 .. (where they fit; zero vectors past n), w = 3 e_1: every product and sum is a small integer, nothing
    rounds.  h_0 == 3, every later scalar and ||w||^2 == 0 exactly, w comes back all zeros (scale_rsqrt leaves a vanished w alone)."""
    V = np.zeros((i + 2, n))
    for k in range(min(i + 1, n)):
        V[k, k] = 1.0
    V[i + 1, :] = 0.0
    V[i + 1, 0] = 3.0
    h = np.zeros(i + 2)
    h[0] = 3.0
    return V, h


def chain_random(n, i, seed):
    """i + 1 seeded basis vectors of norm about 1 (not orthogonal: the single steps are what is checked) and a seeded w."""
    V = np.random.default_rng(seed).standard_normal((i + 2, n))
    V[:i + 1] /= np.sqrt(n)
    return V


# ---- restatements in plain fp64, in the kernels' order ---------------------------------------------------------------------------------------
def _block_sum(acc):
    """block_sum of mg_kernels.hpp for acc[nb, BLK]: the xor butterfly inside each wavefront (lane 0's value), then the waves in turn."""
    a = acc.reshape(acc.shape[0], BLK // 64, 64)
    w = 64
    while w > 1:
        w //= 2
        a = a[..., :w] + a[..., w:2 * w]
    s = np.zeros(acc.shape[0])
    for wv in range(BLK // 64):
        s = s + a[:, wv, 0]
    return s


def _grid_stride(terms, lanes):
    """acc[lane] += terms[lane], terms[lane + lanes], ... in that order."""
    trips = -(-terms.size // lanes)
    t = np.zeros(trips * lanes)
    t[:terms.size] = terms
    acc = np.zeros(lanes)
    for row in t.reshape(trips, lanes):
        acc = acc + row
    return acc


def _sum_final(partial):
    return float(_block_sum(_grid_stride(partial, BLK).reshape(1, BLK))[0])


def reduction_blocks(n):
    return min(NRED_BLOCKS, max(1, (n // 2 + BLK - 1) // BLK))


def grid_for(total):
    return max(1, min((total + BLK - 1) // BLK, GRID_CAP))


def model_dot(x, y, drop_tail=False, drop_last_partial=False):
    """dot_partial + sum_final: pairs grid-stride, the odd tail on lane 0 of workgroup 0, per-workgroup partials, the final sum."""
    n = x.size
    n2, nb = n // 2, reduction_blocks(n)
    pairs = x[0:2 * n2:2] * y[0:2 * n2:2] + x[1:2 * n2:2] * y[1:2 * n2:2]
    acc = _grid_stride(pairs, nb * BLK)
    if n % 2 == 1 and not drop_tail:
        acc[0] = acc[0] + x[n - 1] * y[n - 1]
    partial = _block_sum(acc.reshape(nb, BLK))
    if drop_last_partial:
        partial = partial[:-1]
    return _sum_final(partial)


def model_sumsq(x, **wrong):
    return model_dot(x, x, **wrong)


def model_norm(x, **wrong):
    return float(np.sqrt(model_dot(x, x, **wrong)))


def model_axpby(a, x, b, y, read_y=False):
    return a * x if (b == 0.0 and not read_y) else a * x + b * y


def model_cg_update(alpha, p, Ap, x, r, with_norm, wrong_sign=False, drop_last_partial=False):
    """cg_update_xr / cg_update_xr_norm: one element per lane and trip, ||r||^2 partials of the new r in the same pass."""
    xn = x + alpha * p
    rn = r + alpha * Ap if wrong_sign else r - alpha * Ap
    if not with_norm:
        return xn, rn, None
    nb = min(grid_for(x.size), NRED_BLOCKS)
    partial = _block_sum(_grid_stride(rn * rn, nb * BLK).reshape(nb, BLK))
    if drop_last_partial:
        partial = partial[:-1]
    return xn, rn, float(np.sqrt(_sum_final(partial)))


def model_cg_p(beta, z, p, swapped=False):
    return beta * z + p if swapped else beta * p + z


def model_mgs_step(hk, v, w, u, old_w_in_sum=False, drop_last_partial=False):
    """mgs_step + sum_final: one element per lane and trip over the reductions' grid."""
    a = -hk
    wn = a * v + 1.0 * w
    nb = reduction_blocks(w.size)
    other = (w if old_w_in_sum else wn) if u is None else u
    partial = _block_sum(_grid_stride(wn * other, nb * BLK).reshape(nb, BLK))
    if drop_last_partial:
        partial = partial[:-1]
    return wn, _sum_final(partial)


def model_chain(V, i, divide_by_zero=False):
    """FgmresCore::arnoldi's chain on V[i + 2, n] (w = the last row, updated in place): returns (h_0 .. h_i, ||w||^2)."""
    w = V[i + 1]
    h = np.zeros(i + 2)
    h[0] = model_dot(w, V[0])
    for k in range(i + 1):
        w[:], h[k + 1] = model_mgs_step(h[k], V[k], w, V[k + 1] if k < i else None)
    nrm = np.sqrt(h[i + 1])
    if nrm != 0.0 or divide_by_zero:
        with np.errstate(all="ignore"):
            w[:] = (1.0 / nrm) * w
    return h


def model_dscale(d, b, row_by_pair=False, drop_tail=False):
    """dscale_kernel for a block on a 16-byte boundary: nrhs == 1 in pairs + tail, even nrhs in pairs with d[i / h], else by element."""
    n, nrhs = b.shape
    total, bf = n * nrhs, b.reshape(-1)
    out = np.full(total, np.nan)
    if nrhs == 1:
        n2 = total // 2
        out[:2 * n2] = d[:2 * n2] * bf[:2 * n2]
        if total % 2 == 1 and not drop_tail:
            out[total - 1] = d[total - 1] * bf[total - 1]
    elif nrhs % 2 == 0:
        i = np.arange(total // 2)
        dd = d[i // nrhs] if row_by_pair else d[i // (nrhs // 2)]
        out[0::2], out[1::2] = dd * bf[0::2], dd * bf[1::2]
    else:
        out[:] = d[np.arange(total) // nrhs] * bf
    return out.reshape(n, nrhs)


def model_xpdr(x, d, r, **wrong):
    out = model_dscale(d, r, **wrong)
    return x + out


def model_gram(X, Y, shift_column=False, drop_last_partial=False):
    """blk_gram_partial (one row per lane and trip, workgroup (p, a) holds row a of its partial) + blk_gram_final (partials in turn)."""
    n, k = X.shape
    nb = min(GRAM_CAP, max(1, (n + BLK - 1) // BLK))
    G = np.zeros((k, k))
    for a in range(k):
        for b in range(k):
            partial = _block_sum(_grid_stride(X[:, a] * Y[:, b], nb * BLK).reshape(nb, BLK))
            t = 0.0
            for p in (partial[:-1] if drop_last_partial else partial):
                t = t + p
            G[a, b] = t
    if shift_column:
        G = np.roll(G, 1, axis=1)
    return G


def model_comb(add, s, inp, Cm, transposed=False, write_through=False):
    """blk_comb: o = s * add (0 without add), then o += in[i, a] * C[a, b] for a in turn.  write_through: the hazard of out == in when
    a row is not read whole before its first entry is written."""
    n, k = inp.shape
    Cu = Cm.T if transposed else Cm
    o = s * add if add is not None else np.zeros((n, k))
    if not write_through:
        for a in range(k):
            o = o + inp[:, a:a + 1] * Cu[a:a + 1, :]
        return o
    row = inp.copy()
    for b in range(k):
        t = o[:, b]
        for a in range(k):
            t = t + row[:, a] * Cu[a, b]
        row[:, b] = t
    return row
