"""-m gpu: the ComplexF64 Krylov drivers on the MI355X (mg_bicgstab_CFP64 / mg_fgmres_CFP64 on a system operator of their own,
mg_cycle_dev_CFP64) against the complex oracle (tests/complex_krylov_oracle.py) on the same host-built hierarchy, and their fused
vector passes (csrc/mg_cxvec.hpp, mg_cvec_*_dev_CFP64) on their own against numpy in long double.

Drivers: flag, count and resvec length equal the oracle's; resvec within 1e-8 * resvec[0], x within 1e-8 * max|x_oracle|, true
residual below 1e-8 (the tolerances of tests/test_krylov.py).  Passes: derived bounds, see test_complex_passes_vs_long_double."""
import ctypes as C

import numpy as np
import pytest
import torch

import complex_krylov_oracle as ck
import complex_oracle as corc
from complex_cases import complex_rhs, helmholtz

pytestmark = pytest.mark.gpu

MG_ERR_INVALID, MG_ERR_STATE = 1, 3
LD = np.longdouble
U = LD(2.0) ** -53


# ---- the fused passes alone -----------------------------------------------------------------------------------------------------
def _ld(t):
    a = t.detach().cpu().numpy()
    return a.real.astype(LD), a.imag.astype(LD)


def _cvecs(n, count, seed):
    """`count` seeded complex128 device vectors of n values with both parts non-zero, on a 16-byte boundary."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    out = [torch.randn(n, dtype=torch.complex128, device="cuda", generator=g) for _ in range(count)]
    assert all(v.data_ptr() % 16 == 0 for v in out)
    return out


def _hu(m):
    """half an ulp of the fp64 numbers of magnitude m"""
    return LD(0.5) * np.spacing(np.asarray(m, dtype=np.float64)).astype(LD)


def _mx(*arrs):
    m = np.abs(arrs[0])
    for a in arrs[1:]:
        m = np.maximum(m, np.abs(a))
    return m


def _cm(c, z):
    """The plain four-multiply product c z in long double: ((re, im), (largest magnitude among the two products and the result of re,
    the same of im))."""
    c = complex(c)
    p1, p2, p3, p4 = LD(c.real) * z[0], LD(c.imag) * z[1], LD(c.real) * z[1], LD(c.imag) * z[0]
    re, im = p1 - p2, p3 + p4
    return (re, im), (_mx(p1, p2, re), _mx(p3, p4, im))


def _close_vec(name, got, ref, count, mag, extra=(0, 0)):
    """Per part: |got - ref| <= count * half an ulp of the largest magnitude among the part's terms, partial results and result
    (+ extra: roundings carried through a later product, bicg_p)."""
    g = _ld(got)
    worst = 0.0
    for part in (0, 1):
        err = np.abs(g[part] - ref[part])
        bound = count * _hu(_mx(mag[part], ref[part])) + extra[part]
        worst = max(worst, float((err / bound).max()))
    print(f"    {name}: worst error {worst:.3f} of its bound ({count} roundings)")
    assert worst <= 1.0, (name, worst)


def _close_sum(name, got, *terms):
    """|got - sum| <= (number of real products) * 2^-53 * sum|terms| (any order of summation of fp64 products)."""
    t = np.concatenate(terms)
    ref, bound = t.sum(), t.size * U * np.abs(t).sum()
    err = abs(LD(got) - ref)
    print(f"    {name}: |sum - reference| = {float(err):.3e} (bound {float(bound):.3e})")
    assert err <= bound, (name, float(err), float(bound))


def _dot_terms(a, b):
    """the 2n real products of each part of dot(a, b) = sum conj(a_i) b_i"""
    return (a[0] * b[0], a[1] * b[1]), (a[0] * b[1], -a[1] * b[0])


def _passes(D, n, check=True):
    """Every fused pass once on fresh seeded vectors; returns {name: (tensors written, sums)}, checked against long double when
    `check` is set (the rerun for the bit comparison is not checked again)."""
    ws = torch.zeros(D.KRV_WORKSPACE, dtype=torch.float64, device="cuda")
    out = torch.zeros(8, dtype=torch.float64, device="cuda")
    alpha, beta, omega = 0.37 - 0.61j, -1.3 + 0.45j, 0.81 + 0.29j
    res = {}

    def sums(k):
        torch.cuda.synchronize()
        return out[:k].cpu().numpy().copy()

    a, b, c = _cvecs(n, 3, 1)
    for xs, ys in (([a, a, c], [b, a, b]), ([a, a, c, b], [b, a, b, c])):
        D.cvec_dots(xs, ys, n, ws, out)
        s = sums(2 * len(xs))
        for j, (x, y) in enumerate(zip(xs, ys) if check else ()):
            re, im = _dot_terms(_ld(x), _ld(y))
            _close_sum(f"dots{len(xs)}[{j}] re", s[2 * j], *re)
            _close_sum(f"dots{len(xs)}[{j}] im", s[2 * j + 1], *im)
        res[f"dots{len(xs)}"] = ([], s)

    x, y = _cvecs(n, 2, 5)
    D.cvec_scale(alpha, x, y, n)
    torch.cuda.synchronize()
    if check:
        ref, mag = _cm(alpha, _ld(x))
        _close_vec("scale", y, ref, 3, mag)
    res["scale"] = ([y.clone()], np.zeros(0))

    r, v, p = _cvecs(n, 3, 6)
    p0, r0 = (_ld(p), _ld(r)) if check else (None, None)
    D.cvec_bicg_p(beta, omega, r, v, p, n)
    torch.cuda.synchronize()
    if check:
        ov, mov = _cm(omega, _ld(v))
        q = (p0[0] - ov[0], p0[1] - ov[1])                       # 4 roundings per part, at magnitude mq ...
        mq = (_mx(mov[0], p0[0], q[0]), _mx(mov[1], p0[1], q[1]))
        bq, mbq = _cm(beta, q)                                   # ... carried through the product with beta
        eq = (4 * _hu(mq[0]), 4 * _hu(mq[1]))
        extra = (abs(beta.real) * eq[0] + abs(beta.imag) * eq[1], abs(beta.real) * eq[1] + abs(beta.imag) * eq[0])
        _close_vec("bicg_p", p, (r0[0] + bq[0], r0[1] + bq[1]), 4, (_mx(mbq[0], r0[0]), _mx(mbq[1], r0[1])), extra)
    res["bicg_p"] = ([p.clone()], np.zeros(0))

    v, r = _cvecs(n, 2, 7)
    r0 = _ld(r) if check else None
    D.cvec_bicg_s(alpha, v, r, n, ws, out)
    s = sums(1)
    if check:
        av, mav = _cm(alpha, _ld(v))
        _close_vec("bicg_s", r, (r0[0] - av[0], r0[1] - av[1]), 4, (_mx(mav[0], r0[0]), _mx(mav[1], r0[1])))
        rd = _ld(r)
        _close_sum("bicg_s ||s||^2", s[0], rd[0] * rd[0], rd[1] * rd[1])
    res["bicg_s"] = ([r.clone()], s)

    t, sv = _cvecs(n, 2, 8)
    D.cvec_bicg_ts(t, sv, n, ws, out)
    s = sums(3)
    if check:
        td = _ld(t)
        re, im = _dot_terms(td, _ld(sv))
        _close_sum("bicg_ts dot(t,s) re", s[0], *re)
        _close_sum("bicg_ts dot(t,s) im", s[1], *im)
        _close_sum("bicg_ts dot(t,t)", s[2], td[0] * td[0], td[1] * td[1])
    res["bicg_ts"] = ([], s)

    phat, shat, t, rtld, x, r = _cvecs(n, 6, 9)
    x0, r0 = (_ld(x), _ld(r)) if check else (None, None)
    D.cvec_bicg_xr(alpha, omega, phat, shat, t, rtld, x, r, n, ws, out)
    s = sums(3)
    if check:
        ap, map_ = _cm(alpha, _ld(phat))
        os_, mos = _cm(omega, _ld(shat))
        upd = (ap[0] + os_[0], ap[1] + os_[1])
        _close_vec("bicg_xr x", x, (x0[0] + upd[0], x0[1] + upd[1]), 8,
                   (_mx(map_[0], mos[0], upd[0], x0[0]), _mx(map_[1], mos[1], upd[1], x0[1])))
        ot, mot = _cm(omega, _ld(t))
        _close_vec("bicg_xr r", r, (r0[0] - ot[0], r0[1] - ot[1]), 4, (_mx(mot[0], r0[0]), _mx(mot[1], r0[1])))
        rd = _ld(r)
        _close_sum("bicg_xr ||r||^2", s[0], rd[0] * rd[0], rd[1] * rd[1])
        re, im = _dot_terms(_ld(rtld), rd)
        _close_sum("bicg_xr dot(rtld,r) re", s[1], *re)
        _close_sum("bicg_xr dot(rtld,r) im", s[2], *im)
    res["bicg_xr"] = ([x.clone(), r.clone()], s)

    for m in (3, 10):        # one pass / two passes of 8 vectors at most
        vs = _cvecs(n, m + 1, 10 + m)
        w, vs = vs[0], vs[1:]
        rng = np.random.default_rng(20 + m)
        h = rng.standard_normal(m) + 1j * rng.standard_normal(m)
        if check:
            ref = _ld(w)
            mag = (np.abs(ref[0]), np.abs(ref[1]))
            for hj, vj in zip(h, vs):
                hv, mhv = _cm(hj, _ld(vj))
                ref = (ref[0] - hv[0], ref[1] - hv[1])
                mag = (_mx(mag[0], mhv[0], ref[0]), _mx(mag[1], mhv[1], ref[1]))
        D.cvec_gs_update(h, vs, w, n, ws, out)
        s = sums(1)
        if check:
            _close_vec(f"gs_update m={m}", w, ref, 4 * m, mag)
            wd = _ld(w)
            _close_sum(f"gs_update m={m} ||w||^2", s[0], wd[0] * wd[0], wd[1] * wd[1])
        res[f"gs_update{m}"] = ([w.clone()], s)
    return res


# the grid of a pass is ceil(n / 1024) workgroups, 1024 at most: 1024 * 1024 + 3 is just past the size at which it reaches that cap
# (lanes of the first workgroups take a fifth trip)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4913, 1024 * 1024 + 3])
def test_complex_passes_vs_long_double(mg, built, n):
    """Seeded complex vectors and scalars with both parts non-zero.  Every sum is within (number of real products summed) * 2^-53 *
    sum|terms| of the long-double sum (2n products per part of a complex dot and per norm).  Every updated element's real and
    imaginary part is within (roundings of the unfused expression) * half an ulp of the largest magnitude among its terms, partial
    results and result.  The expressions are the ones csrc/mg_cxvec.hpp writes, c z = (c.x z.x - c.y z.y) + i (c.x z.y + c.y z.x)
    first (3 roundings per part), then the sums; FMA contraction can only drop roundings:
      scale      y = a x                                      3
      bicg_s     r - alpha v                                  3 + 1 = 4
      bicg_xr    x + (alpha phat + omega shat)                3 + 3 + 1 + 1 = 8;   r - omega t: 4
      gs_update  w - h_1 v_1 - ... - h_m v_m, in that order   4 m (magnitudes of every step)
      bicg_p     r + beta (p - omega v)                       8: 4 of the product with beta and the final sum, and 4 of
                 q = p - omega v, which the product with beta carries on - those are charged |beta.x| and |beta.y| times half an
                 ulp of the largest magnitude inside q (q may cancel, so the magnitudes of beta q do not cover them).
    Two runs are bit-identical."""
    D = mg.device
    D.load_library()
    print(f"  n = {n}")
    first = _passes(D, n)
    second = _passes(D, n, check=False)
    for name, (tensors, s) in first.items():
        t2, s2 = second[name]
        assert np.array_equal(s, s2), (name, s, s2)                       # bit-identical sums ...
        for u, v in zip(tensors, t2):
            assert torch.equal(u, v), name                                # ... and vectors


def test_complex_passes_refuse_misaligned_vectors(mg, built):
    """A complex vector 8 bytes off a 16-byte boundary (a sliced float view): MG_ERR_INVALID from every pass, nothing is launched."""
    D = mg.device
    D.load_library()
    n = 64
    base = torch.zeros(2 * n + 2, dtype=torch.float64, device="cuda")
    off = int(base.data_ptr()) + 8
    good = _cvecs(n, 8, 3)
    keep = [g.clone() for g in good]
    ws = torch.zeros(D.KRV_WORKSPACE, dtype=torch.float64, device="cuda")
    out = torch.zeros(8, dtype=torch.float64, device="cuda")
    g = good
    calls = [lambda: D.cvec_dots([g[0], off], [g[1], g[2]], n, ws, out),
             lambda: D.cvec_scale(1 + 1j, g[0], off, n),
             lambda: D.cvec_bicg_p(1 + 1j, 1 - 1j, g[0], off, g[1], n),
             lambda: D.cvec_bicg_s(1 + 1j, off, g[0], n, ws, out),
             lambda: D.cvec_bicg_ts(g[0], off, n, ws, out),
             lambda: D.cvec_bicg_xr(1 + 1j, 1 - 1j, g[0], g[1], g[2], off, g[3], g[4], n, ws, out),
             lambda: D.cvec_gs_update([1 + 1j, 2 - 1j], [g[0], off], g[1], n, ws, out)]
    for call in calls:
        with pytest.raises(D.MGDeviceError, match=rf"status {MG_ERR_INVALID}\b.*16-byte"):
            call()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(good, keep)) and not base.any()


# ---- the drivers against the oracle ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def devs(mg, built):
    """One device hierarchy per case with its system operator set, shared by the tests below."""
    made = {}

    def get(name):
        if name not in made:
            p, As, _ = ck.case(mg, name)
            made[name] = mg.device.DeviceHierarchy(p)
            made[name].set_krylov_operator(As)
        return made[name]

    yield get
    for d in made.values():
        d.close()


def _check_run(tag, got, ref, As, b, residual=True):
    x, flag, it, rv = got
    xo, fo, ito, rvo = ref
    dr = np.abs(rv - rvo[: len(rv)]).max() / rvo[0] if len(rv) else 0.0
    dx = np.abs(x - xo).max() / np.abs(xo).max()
    res = np.linalg.norm(b - As @ x) / np.linalg.norm(b)
    print(f"  {tag}: flag {flag} ({fo}), count {it} ({ito}), resvec diff {dr:.2e}, x diff {dx:.2e}, true residual {res:.3e}")
    assert (flag, it, len(rv)) == (fo, ito, len(rvo))
    assert dr <= 1e-8 and dx <= 1e-8
    if residual:
        assert res < 1e-8


@pytest.mark.parametrize("name", ["C1", "C2", "C3"])
def test_bicgstab_against_oracle(mg, devs, name):
    p, As, b = ck.case(mg, name)
    x = np.zeros_like(b)
    got = devs(name).bicgstab(b, x, ck.TOL, ck.MAXIT_BICGSTAB)
    assert got[0] is x
    _check_run(f"{name} BiCGSTAB", got, ck.reference(mg, name, "bicgstab"), As, b)
    assert (got[2], got[1]) == ck.EXPECTED[name]["bicgstab"]


@pytest.mark.parametrize("name,inner", [("C1", 5), ("C1", 10), ("C2", 10), ("C3", 5), ("C3", 10)])
def test_fgmres_against_oracle(mg, devs, name, inner):
    """Restarts are exercised: C1 with inner = 5 takes 57 steps, 12 restart cycles."""
    p, As, b = ck.case(mg, name)
    x = np.zeros_like(b)
    got = devs(name).fgmres(b, x, inner, ck.TOL, ck.MAXIT_FGMRES)
    _check_run(f"{name} FGMRES({inner})", got, ck.reference(mg, name, "fgmres", inner), As, b)
    assert got[2] == ck.EXPECTED[name][inner] and got[1] == 0


def test_driver_edges_on_c3(mg, devs):
    p, As, b = ck.case(mg, "C3")
    dev = devs("C3")
    n = b.shape[0]
    run_b = lambda x0, maxit=ck.MAXIT_BICGSTAB, rhs=b: dev.bicgstab(rhs, x0, ck.TOL, maxit)
    run_g = lambda x0, maxit=ck.MAXIT_FGMRES, rhs=b: dev.fgmres(rhs, x0, 5, ck.TOL, maxit)
    # x0 != 0: the first oracle iterate
    x1b = ck.reference(mg, "C3", "bicgstab", maxIter=1, key="first")[0]
    _check_run("BiCGSTAB from x1", run_b(x1b.copy()), ck.reference(mg, "C3", "bicgstab", x0=x1b, key="from-x1"), As, b)
    x1g = ck.reference(mg, "C3", "fgmres", 5, maxIter=1, key="first")[0]
    _check_run("FGMRES(5) from x1", run_g(x1g.copy()), ck.reference(mg, "C3", "fgmres", 5, x0=x1g, key="from-x1"), As, b)
    # b = 0: flag -9, x zero
    for run in (run_b, run_g):
        x, flag, it, rv = run(complex_rhs(n, 3), rhs=np.zeros_like(b))
        assert flag == -9 and it == 0 and len(rv) == 0 and not x.any()
    # maxIter = 3: flag -1, the oracle's prefix
    ref = ck.reference(mg, "C3", "bicgstab", maxIter=3, key="three")
    assert (ref[1], ref[2], len(ref[3])) == (-1, 3, 7)
    _check_run("BiCGSTAB maxIter 3", run_b(np.zeros_like(b), 3), ref, As, b, residual=False)
    assert np.abs(ref[3] - ck.reference(mg, "C3", "bicgstab")[3][:7]).max() == 0.0
    ref = ck.reference(mg, "C3", "fgmres", 5, maxIter=3, key="three")
    assert (ref[1], ref[2], len(ref[3])) == (-1, 15, 15)
    _check_run("FGMRES(5) maxIter 3", run_g(np.zeros_like(b), 3), ref, As, b, residual=False)
    # two runs of each driver are bit-identical; the _dev entry points on torch.complex128 tensors equal them bit for bit
    for run, run_dev in ((run_b, lambda bt, xt: dev.bicgstab_dev(bt, xt, ck.TOL, ck.MAXIT_BICGSTAB)),
                         (run_g, lambda bt, xt: dev.fgmres_dev(bt, xt, 5, ck.TOL, ck.MAXIT_FGMRES))):
        r1, r2 = run(np.zeros_like(b)), run(np.zeros_like(b))
        assert np.array_equal(r1[0], r2[0]) and r1[1:3] == r2[1:3] and np.array_equal(r1[3], r2[3])
        bt, xt = torch.from_numpy(b).cuda(), torch.zeros(n, dtype=torch.complex128, device="cuda")
        flag, it, rv = run_dev(bt, xt)
        assert (flag, it) == r1[1:3] and np.array_equal(rv, r1[3]) and np.array_equal(xt.cpu().numpy(), r1[0])
        assert np.array_equal(bt.cpu().numpy(), b)
    with pytest.raises(TypeError):
        dev.bicgstab(b.real.copy(), np.zeros(n), ck.TOL, 3)
    with pytest.raises(TypeError):
        dev.fgmres_dev(torch.zeros(2 * n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.complex128, device="cuda"), 5, ck.TOL, 3)


def test_no_krylov_operator_is_the_fine_level(mg, built):
    """No Krylov operator set, the operator cleared again, and A = As[0] uploaded as one: the same bits."""
    p, As, b = ck.case(mg, "C3")
    dev = mg.device.DeviceHierarchy(p)
    try:
        def both():
            rb = dev.bicgstab(b, np.zeros_like(b), ck.TOL, ck.MAXIT_BICGSTAB)
            rg = dev.fgmres(b, np.zeros_like(b), 5, ck.TOL, ck.MAXIT_FGMRES)
            return rb, rg

        unset = both()
        dev.set_krylov_operator(p.As[0])
        as0 = both()
        dev.set_krylov_operator(As)
        other = both()
        dev.set_krylov_operator(None)
        cleared = both()
        for k in (0, 1):
            assert unset[k][1] in (0, -3)
            assert np.linalg.norm(b - p.As[0] @ unset[k][0]) / np.linalg.norm(b) < 1e-8
            for alt in (as0, cleared):
                assert np.array_equal(unset[k][0], alt[k][0]) and unset[k][1:3] == alt[k][1:3] and np.array_equal(unset[k][3], alt[k][3])
            assert not np.array_equal(unset[k][0], other[k][0])            # (the other operator was really applied)
    finally:
        dev.close()


def test_cycle_dev_equals_host_cycle(mg, devs):
    p, As, b = ck.case(mg, "C3")
    dev = devs("C3")
    n = b.shape[0]
    x = np.zeros_like(b)
    dev.cycle(b, x, 1)
    bt, xt = torch.from_numpy(b).cuda(), torch.zeros(n, dtype=torch.complex128, device="cuda")
    dev.cycle_dev(bt, xt, 1)
    torch.cuda.synchronize()
    assert np.array_equal(xt.cpu().numpy(), x)
    xo = corc.recursiveCycle(p, b, np.zeros_like(b), 1)
    assert np.abs(x - xo).max() <= 1e-12 * np.abs(xo).max()
    dev.cycle(b, x, 0)                                                   # from x != 0
    dev.cycle_dev(bt, xt, 0)
    torch.cuda.synchronize()
    assert np.array_equal(xt.cpu().numpy(), x) and np.array_equal(bt.cpu().numpy(), b)


@pytest.mark.parametrize("krylov", ["GMRES", "BiCGSTAB"])
def test_wrapper_routes_complex_solvers(mg, built, krylov):
    A, mesh = helmholtz(mg, [16] * 3, 0.5, 0.5)
    p = mg.getMGparam(np.complex128, np.int64, 3, 8, 30, 1e-8, "SPAI", 1.0, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
    s = mg.getMGsolver(p, mesh, 2, krylov)
    B = complex_rhs(A.shape[0], 31)
    X = np.zeros_like(B)
    try:
        mg.solveLinearSystem_(A, B, X, s)
        res = np.linalg.norm(A @ X - B) / np.linalg.norm(B)
        print(f"  {krylov}: {s.nIter} iterations, flag {p.flag}, ||A X - B|| / ||B|| = {res:.3e}")
        assert p.flag in (0, -3) and s.nIter > 0 and res < s.tol
    finally:
        mg.clear_(p)


def test_both_routes_to_the_krylov_operator_agree(mg, built):
    """The system operator can be set on the device hierarchy (set_krylov_operator) and by the solve functions (their A, uploaded
    when it is not the object uploaded last).  Whichever route set it last, a solve applies the operator it was asked for: the true
    residual is checked against THAT operator (the other one's solution leaves a residual of the order of 1e-1)."""
    Ah, mesh = helmholtz(mg, [8] * 3, 0.5, 0.5)
    As, _ = helmholtz(mg, [8] * 3, 0.5, 0.05)
    p = mg.getMGparam(np.complex128, np.int64, 2, 8, 40, 1e-8, "SPAI", 1.0, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(Ah, mesh, p)
    b = complex_rhs(Ah.shape[0], 21)
    res = lambda A, x: np.linalg.norm(b - A @ x) / np.linalg.norm(b)

    def solved(A, x, other):
        print(f"    residual against the intended operator {res(A, x):.3e}, against the other {res(other, x):.3e}")
        assert p.flag in (0, -3) and res(A, x) < 1e-8 and res(other, x) > 1e-4

    try:
        dev = mg.to_device(p)
        assert dev.krylov_operator is None
        dev.set_krylov_operator(As)                                       # set on the device ...
        assert dev.krylov_operator is As
        x = np.zeros_like(b)
        mg.solveBiCGSTAB_MG_CFP64(None, p, b, x)                          # ... a solve on the fine level clears it
        assert dev.krylov_operator is None
        solved(p.As[0], x, As)
        x = np.zeros_like(b)
        mg.solveGMRES_MG_CFP64(As, p, b, x, True, 5)                      # uploaded by the solve function ...
        assert dev.krylov_operator is As
        solved(As, x, p.As[0])
        dev.set_krylov_operator(None)                                     # ... cleared on the device ...
        x = np.zeros_like(b)
        mg.solveGMRES_MG_CFP64(As, p, b, x, True, 5)                      # ... and uploaded again, not skipped
        assert dev.krylov_operator is As
        solved(As, x, p.As[0])
        s = mg.getMGsolver(p, mesh, 2, "BiCGSTAB")                        # the wrapper solves with As[0] whatever was set before
        x = np.zeros_like(b)
        mg.solveLinearSystem_(p.As[0], b, x, s)
        assert dev.krylov_operator is None
        solved(p.As[0], x, As)
        x = np.zeros_like(b)
        mg.solveBiCGSTAB_MG_CFP64(p.As[0], p, b, x)                       # As[0] itself: the fine level, nothing to upload
        assert dev.krylov_operator is None
        solved(p.As[0], x, As)
    finally:
        mg.clear_(p)


def test_refusals_leave_the_handle_usable(mg, devs):
    lib = mg.device.load_library()
    p, As, b = ck.case(mg, "C3")
    dev = devs("C3")
    n = b.shape[0]
    A8, mesh8 = mg.poisson_shifted([8, 8, 8])
    pr = mg.getMGparam(np.float64, np.int64, 2, 8, 4, 1e-10, "Jac", 0.8, 1, 1, "V")
    mg.MGsetup(A8, mesh8, pr)
    rdev = mg.device.DeviceHierarchy(pr)
    raw = C.c_void_p()
    assert lib.mg_create_CF64(2, 1, 0, C.byref(raw)) == 0                 # a CF64 handle that is never finalized
    try:
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_longlong)
        hb, hx = np.zeros(2 * n), np.zeros(2 * n)
        tb, tx = torch.zeros(2 * n, dtype=torch.float64, device="cuda"), torch.zeros(2 * n, dtype=torch.float64, device="cuda")
        hp = lambda a: a.ctypes.data_as(dp)
        lz = C.c_longlong(0)
        lp = C.byref(lz)
        M = As.tocsr()
        cp = np.ascontiguousarray(M.indptr, dtype=np.int64) + 1
        rv = np.ascontiguousarray(M.indices, dtype=np.int64) + 1
        nz = np.ascontiguousarray(np.conj(M.data)).view(np.float64)
        li = lambda a: a.ctypes.data_as(ip)

        def refused(rc, code, fragment):
            """the status, and in mg_last_error the message of THIS refusal (each kind has a fragment of its own)"""
            msg = (lib.mg_last_error() or b"").decode()
            assert rc == code, (rc, msg)
            assert fragment in msg, (fragment, msg)

        def all_entries(h, nn, code, fragment):
            refused(lib.mg_set_krylov_operator_CFP64_INT64(h, nn, li(cp), li(rv), hp(nz)), code, fragment)
            refused(lib.mg_cycle_dev_CFP64(h, tb.data_ptr(), tx.data_ptr(), nn, 1), code, fragment)
            refused(lib.mg_bicgstab_CFP64(h, hp(hb), hp(hx), nn, 1e-6, 3, lp, lp, hp(hb), lp), code, fragment)
            refused(lib.mg_bicgstab_dev_CFP64(h, tb.data_ptr(), tx.data_ptr(), nn, 1e-6, 3, lp, lp, hp(hb), lp), code, fragment)
            refused(lib.mg_fgmres_CFP64(h, hp(hb), hp(hx), nn, 5, 1e-6, 3, lp, lp, hp(hb), lp), code, fragment)
            refused(lib.mg_fgmres_dev_CFP64(h, tb.data_ptr(), tx.data_ptr(), nn, 5, 1e-6, 3, lp, lp, hp(hb), lp), code, fragment)

        all_entries(rdev.handle, n, MG_ERR_STATE, "on an FP64 handle")    # an FP64 handle
        all_entries(raw, n, MG_ERR_STATE, "not finalized")                # a CF64 handle before mg_finalize ...
        assert lib.mg_set_krylov_operator_CFP64_INT64(raw, n, None, None, None) == 0   # ... on which the operator can still be cleared
        hc = dev.handle
        for inner in (0, 65):
            refused(lib.mg_fgmres_CFP64(hc, hp(hb), hp(hx), n, inner, 1e-6, 3, lp, lp, hp(hb), lp), MG_ERR_INVALID, "inner must be")
            refused(lib.mg_fgmres_dev_CFP64(hc, tb.data_ptr(), tx.data_ptr(), n, inner, 1e-6, 3, lp, lp, hp(hb), lp), MG_ERR_INVALID,
                    "inner must be")
        refused(lib.mg_bicgstab_CFP64(hc, None, hp(hx), n, 1e-6, 3, lp, lp, hp(hb), lp), MG_ERR_INVALID, "null vector")
        refused(lib.mg_bicgstab_CFP64(hc, hp(hb), hp(hx), n, 1e-6, -1, lp, lp, hp(hb), lp), MG_ERR_INVALID, "maxIter < 0")
        refused(lib.mg_fgmres_CFP64(hc, hp(hb), hp(hx), n + 1, 5, 1e-6, 3, lp, lp, hp(hb), lp), MG_ERR_INVALID, "does not match the fine level")
        refused(lib.mg_cycle_dev_CFP64(hc, tb.data_ptr(), tx.data_ptr(), n, -1), MG_ERR_INVALID, "x_is_zero")
        refused(lib.mg_bicgstab_dev_CFP64(hc, tb.data_ptr() + 8, tx.data_ptr(), n, 1e-6, 3, lp, lp, hp(hb), lp), MG_ERR_INVALID, "16-byte")
        Ah, _ = helmholtz(mg, [4] * 3, 0.5, 0.05)                         # a Krylov operator of the wrong order
        with pytest.raises(mg.device.MGDeviceError, match=rf"status {MG_ERR_INVALID}\b.*Krylov operator of order 125"):
            dev.set_krylov_operator(Ah)
        assert dev.krylov_operator is As                                  # (the refused upload left the operator that was there)
        with pytest.raises(NotImplementedError):
            dev.pcg(b, np.zeros_like(b), 1e-6, 3)
        # the handle still cycles and solves as before
        x = np.zeros_like(b)
        dev.cycle(b, x, 1)
        xo = corc.recursiveCycle(p, b, np.zeros_like(b), 1)
        assert np.abs(x - xo).max() <= 1e-12 * np.abs(xo).max()
        _check_run("BiCGSTAB after the refusals", dev.bicgstab(b, np.zeros_like(b), ck.TOL, ck.MAXIT_BICGSTAB),
                   ck.reference(mg, "C3", "bicgstab"), As, b)
    finally:
        lib.mg_destroy(raw)
        rdev.close()
