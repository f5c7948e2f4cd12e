"""CPU: the ``singleKcycle`` switch, the new entry points' declarations, and the single K-cycle oracle
(tests/complex_single_kcycle_oracle.py) against tests/complex_kcycle_oracle.py - with the conditions on the inputs of
tests/test_complex_single_kcycle_gpu.py asserted on the oracles alone.

Bounds.  The single oracle's cycle on a hierarchy whose data are exactly representable in single against the double oracle's on the same
data: 8 * 2^-24 of max|x| - "a few units": the operators have at most 3 entries per row (a row sum rounds at most 3 times, each by
half a unit of its result), a V(2,2) or K(2,1) cycle on three levels chains about a dozen such products and updates into the largest
entry of x, and their roundings add like a random walk (sqrt(12) * 0.5 < 2 units) unless the oracle does more than the contract allows
- a second rounding of x or Gram scalars in single, which move t by 2^-24 cond(H), show up above it.  Conditions on the inputs: no residual
estimate within a factor 4 of the break's 1e-5, for both oracles; the same `used` in both traces; cond(H) <= 1e5 in the relaxation
cases; e_ref <= 1e-3 in the cycle cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import complex_kcycle_oracle as korc
import complex_single_kcycle_cases as K
import complex_single_kcycle_oracle as sk

C64, C128 = np.complex64, np.complex128
U32 = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the switch ---------------------------------------------------------------------------------------------------------------------------
def test_flag(mg):
    base = (np.complex128, np.int64, 3, 8, 5, 1e-6, "Jac", 0.8, 2, 1, "K")
    assert mg.getMGparam(*base, singlePrecision=True).singleKcycle is False
    assert mg.getMGparam(*base).singleKcycle is False
    p = mg.getMGparam(*base, singlePrecision=True, singleKcycle=True)
    assert p.singleKcycle is True and p.VAL == np.complex64
    q = mg.copySolver(p)
    assert q.singleKcycle is True and q.singlePrecision is True and q.cycleType == "K"
    assert mg.copySolver(mg.getMGparam(*base, singlePrecision=True)).singleKcycle is False
    with pytest.raises(NotImplementedError):
        mg.getMGparam(*base, singleKcycle=True)                   # ComplexF64: served without it
    with pytest.raises(NotImplementedError):
        mg.getMGparam(np.float64, np.int64, 3, 8, 5, 1e-6, "Jac", 0.8, 2, 1, "K", singleKcycle=True)
    with pytest.raises(TypeError):
        mg.getMGparam(*base, "NoMUMPS", 0.4, 0.0, "FullWeighting", True, True)     # keyword only


def test_guards_let_the_flag_through(mg):
    """_vanka_guard: 'K' on a ComplexF32 Vanka param passes with the flag and is refused without it (no device is touched)."""
    from multigrid_jl_amd.device import _vanka_guard
    p = K.vanka_param(mg)
    _vanka_guard(p, 1)
    q = mg.copySolver(p)
    q.singleKcycle = False
    q.Meshes = p.Meshes
    with pytest.raises(NotImplementedError, match="ComplexF64 hierarchies only"):
        _vanka_guard(q, 1)


def test_entry_points_are_exported_declared_and_bound(mg, built):
    lib = mg.device.load_library()
    header = open(os.path.join(ROOT, "include", "mgvcycle.h")).read()
    fp, dp, ll = C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_longlong
    want = {"mg_set_schedule_CF32": [C.c_void_p, ll, ll],
            "mg_fgmres_relax_CF32": [C.c_void_p, ll, fp, fp, ll, ll, C.c_double, dp, dp, dp, C.POINTER(ll), fp, fp]}
    for name, args in want.items():
        fn = getattr(lib, name)                                   # exported
        assert re.search(rf"\bmg_status\s+{name}\s*\(", header)   # declared
        restype, argtypes = mg.device.SIGNATURES[name]            # bound
        assert restype is C.c_int and list(argtypes) == args
        assert fn.restype is C.c_int and list(fn.argtypes) == args
    assert re.search(r"mg_fgmres_relax_CF32\([^;]*float\*\s*Z_out,\s*float\*\s*AZ_out\)", header)
    assert lib.mg_set_schedule_CF32(None, ord("K"), 1) != 0 and lib.mg_last_error()      # (a null handle: refused, not a crash)


# ---- the single oracle on exactly representable data -----------------------------------------------------------------------------------------
def _dyadic_param(mg, relax, cyc, pre, post):
    """Three levels in 1-D (31 -> 15 -> 7 unknowns): A = tridiag(-1, 4 + i, -1), linear interpolation (1/2, 1, 1/2), R = P'/2, Galerkin
    coarse operators, d = 1/4 - i/16 - every value a dyadic rational with a short numerator, exactly representable in single (asserted)."""
    def interp(nc):
        n = 2 * nc + 1
        P = sp.lil_matrix((n, nc))
        for j in range(nc):
            P[2 * j, j], P[2 * j + 1, j], P[2 * j + 2, j] = 0.5, 1.0, 0.5
        return P.tocsr()

    n = 31
    A = sp.diags([-np.ones(n - 1), np.full(n, 4.0 + 1.0j), -np.ones(n - 1)], [-1, 0, 1]).tocsr().astype(C128)
    As, Ps, Rs = [A], [], []
    for nc in (15, 7):
        P = interp(nc)
        R = (0.5 * P.T).tocsr()
        Ps.append(P)
        Rs.append(R)
        As.append((R @ As[-1] @ P).tocsr())
    for M in As + Ps + Rs:
        M.sort_indices()
        assert np.array_equal(M.data.astype(C64 if M.dtype.kind == "c" else np.float32).astype(M.dtype), M.data)   # exact in single
    p = K.single_param(mg, 3, relax, 1.0, pre, post, cyc)
    p.As = [M.astype(C64) for M in As]
    p.Ps = [M.astype(np.float32) for M in Ps]
    p.Rs = [M.astype(np.float32) for M in Rs]
    p.relaxPrecs = [np.full(M.shape[0], 0.25 - 0.0625j, dtype=C64) for M in As[:-1]]
    p.LU = spla.splu(sp.csc_matrix(As[-1]))
    p.nrhs = 1
    return p


@pytest.mark.parametrize("sched", [("Jac-GMRES", "V", 2, 2), ("Jac-GMRES", "K", 2, 1), ("Jac", "K", 2, 1), ("Jac-GMRES", "K", 1, 1)],
                         ids=K.case_id)
def test_single_oracle_on_exactly_representable_data(mg, sched):
    p = _dyadic_param(mg, *sched)
    rng = np.random.default_rng(5)
    b64 = (rng.integers(-16, 17, 31) + 1j * rng.integers(-16, 17, 31)) * 512.0         # integers (|b| ~ 5000 keeps every rn clear of the break at 1e-5)
    b = b64.astype(C64)
    assert np.array_equal(b.astype(C128), b64)
    t64, ts = [], []
    x64, xs = K.cycle_oracles(p, b, np.zeros_like(b), t64, ts)
    assert xs.dtype == C64
    e = K.dist(xs, x64)
    print(f"{sched}: single oracle {e / U32:.2f} units of 2^-24 from the double oracle; used {K.used(ts)}")
    assert len(ts) > 0 and K.used(ts) == K.used(t64)
    assert korc.rn_clear_of_tol(ts, 4.0) and korc.rn_clear_of_tol(t64, 4.0)
    assert e <= 8 * U32
    rn_s, rn_d = korc.all_rn(ts), korc.all_rn(t64)
    assert np.abs(rn_s - rn_d).max() <= 1e-4 * rn_d.max()         # the estimates are double algebra on single data: close, not equal


def test_relaxation_contract_of_the_single_oracle(mg):
    """What the oracle's relaxation is made of: complex64 bases with Z[:,0] = fl(d.*r0), Z[:,j+1] = fl(d.*AZ[:,j]); x = fl(x0 + Z t) with
    t from the double H and xi of those bases."""
    r = K.relax_reference(mg, "oneblock100", 3)
    p = K.relax_param(mg, "oneblock100")
    d = p.relaxPrecs[0]
    Z, AZ = r["Z"], r["AZ"]
    assert Z.dtype == C64 and AZ.dtype == C64 and Z.shape == (100, 3)
    assert np.array_equal(Z[:, 0], d * r["r0"]) and np.array_equal(Z[:, 1], d * AZ[:, 0]) and np.array_equal(Z[:, 2], d * AZ[:, 1])
    t = korc.julia_pinv(r["H"]) @ r["xi"]
    xref = r["x0"].astype(C128) + Z.astype(C128) @ t
    assert np.abs(r["x"].astype(C128) - xref).max() <= 2 * U32 * np.abs(xref).max() + 100 * np.finfo(float).eps * r["cond"] * np.abs(Z.astype(C128) @ t).max()


# ---- the conditions on the inputs of the GPU tests ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inner", K.INNERS)
@pytest.mark.parametrize("name", ["awkward5000", "oneblock100"])
def test_relaxation_inputs(mg, name, inner):
    r = K.relax_reference(mg, name, inner)
    print(f"{name} inner={inner}: cond(H) {r['cond']:.3e}, rn {min(r['rnorms']):.2e} .. {max(r['rnorms']):.2e}")
    assert r["cond"] <= 1e5
    assert len(r["rnorms"]) == inner and min(r["rnorms"]) >= 4e-5              # no break: every direction is used
    p = K.relax_param(mg, name)
    A, d = p.As[0], p.relaxPrecs[0]
    assert A.shape[0] % 256 != 0 and A.dtype == C64 and d.dtype == C64
    assert 0.05 < np.abs(d).mean() < 0.2                                        # |d| ~ 0.1
    if name == "awkward5000":
        m = np.diff(A.indptr)
        assert m[2000] == 3000 and (m == 0).sum() >= 40 and m[100:104].sum() > 1024 and d[2000] != 0 and r["r0"][2000] != 0
    else:
        assert A.nnz < 1024 and A.shape[0] <= 256


def test_break_input(mg):
    r = K.relax_reference(mg, "awkward5000", 3, 1e-9)
    assert len(r["rnorms"]) == 1 and r["rnorms"][0] < 1e-5 / 4


@pytest.mark.parametrize("prob,sched,variant", K.CYCLE_CASES, ids=K.case_id)
def test_cycle_inputs(mg, prob, sched, variant):
    ref = K.cycle_reference(mg, prob, sched, variant)
    t64, ts = ref["trace64"], ref["traces"]
    print(f"{prob} {sched} {variant}: e_ref {ref['e_ref']:.3e}, {len(ts)} relaxations")
    assert len(ts) > 0 and K.used(ts) == K.used(t64)
    assert korc.rn_clear_of_tol(ts, 4.0) and korc.rn_clear_of_tol(t64, 4.0), (korc.all_rn(ts), korc.all_rn(t64))
    assert 0 < ref["e_ref"] <= 1e-3
    assert ref["xs"].dtype == C64
    if variant == "second":
        assert np.abs(ref["x0"]).max() > 0


def test_solve_input(mg):
    ref = K.solve_reference(mg)
    assert korc.rn_clear_of_tol(ref["trace"], 4.0), korc.all_rn(ref["trace"])
    assert korc.rn_clear_of_tol(ref["trace64"], 4.0), korc.all_rn(ref["trace64"])
    assert ref["iters64"] == ref["iters"] and len(ref["trace"]) > 0 and K.used(ref["trace"]) == K.used(ref["trace64"])
    rvo, tolr = ref["resvec"], 4 * ref["e_ref"] * ref["resvec"][0]
    print(f"solveMG input: {ref['iters']} cycles, relres {rvo[-1] / rvo[0]:.3e}, e_ref {ref['e_ref']:.3e}")
    assert ref["iters"] < ref["p"].maxOuterIter
    assert abs(rvo[-1] - ref["p"].relativeTol * rvo[0]) > tolr and abs(rvo[-2] - ref["p"].relativeTol * rvo[0]) > tolr   # the stop is no rounding's decision


@pytest.mark.parametrize("name", list(K.DRIVER_SCHEDS))
def test_driver_inputs(mg, name):
    """The drivers' cases: every residual estimate of every preconditioner call clear of the break, for the single and for the double
    oracle as M, the same `used` in both as far as both runs go, and the oracle's BiCGSTAB ending at a full step with 10% to spare."""
    import complex_krylov_oracle as ck
    ref = K.driver_reference(mg, name)
    for ts, t64 in zip(ref["traces"], ref["traces64"]):
        assert len(ts) > 0 and korc.rn_clear_of_tol(ts, 4.0) and korc.rn_clear_of_tol(t64, 4.0), (korc.all_rn(ts).min(), korc.all_rn(t64).min())
        k = min(len(ts), len(t64))
        assert K.used(ts[:k]) == K.used(t64[:k])
    rvb = ref["bicgstab"][3]
    assert ref["bicgstab"][1] == 0 and ref["fgmres"][1] == 0
    assert rvb[-2] >= 1.1 * ck.TOL and rvb[-1] <= 0.9 * ck.TOL
