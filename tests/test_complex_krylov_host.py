"""ComplexF64 Krylov drivers, host side (no GPU): the exported symbols, the complex oracle (tests/complex_krylov_oracle.py) pinned
to the real one and shown to converge on the cases the GPU tests use, and what the Python layer refuses before it touches a device."""
import os
import re

import numpy as np
import pytest

import complex_krylov_oracle as ck
from oracle import mg_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgvcycle.h")

CVEC = ["mg_cvec_%s_dev_CFP64" % p for p in ("dots", "bicg_p", "bicg_s", "bicg_ts", "bicg_xr", "gs_update", "scale")]
DRIVERS = ["mg_set_krylov_operator_CFP64_INT64", "mg_cycle_dev_CFP64", "mg_bicgstab_CFP64", "mg_bicgstab_dev_CFP64", "mg_fgmres_CFP64",
           "mg_fgmres_dev_CFP64"]


def test_complex_krylov_symbols_declared_exported_and_bound(mg, built):
    """Fails without the feature: the parent's header, library and binding have none of these."""
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\bint\s+(mg_\w+)\s*\(", header))
    lib = mg.device.load_library()
    for n in CVEC + DRIVERS:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in mg.device.SIGNATURES, n
        assert "_CF64" not in n
    for n in ("cvec_dots", "cvec_bicg_p", "cvec_bicg_s", "cvec_bicg_ts", "cvec_bicg_xr", "cvec_gs_update", "cvec_scale"):
        assert callable(getattr(mg.device, n))
    for n in ("set_krylov_operator", "bicgstab", "fgmres", "bicgstab_dev", "fgmres_dev", "cycle_dev"):
        assert getattr(mg.device.ComplexDeviceHierarchy, n) is not mg.device.ComplexDeviceHierarchy._refuse, n
    for n in ("pcg", "pcg_dev", "block_pcg_dev", "block_bicgstab_dev", "block_fgmres_dev", "solve_dev", "spmv_dev"):
        assert getattr(mg.device.ComplexDeviceHierarchy, n) is mg.device.ComplexDeviceHierarchy._refuse, n
    assert callable(mg.solveBiCGSTAB_MG_CFP64) and callable(mg.solveGMRES_MG_CFP64)


@pytest.mark.parametrize("relax,cyc", [("Jac", "V"), ("SPAI", "W")])
def test_complex_oracle_equals_real_oracle_on_real_operator(mg, relax, cyc):
    """Real A, real b: the complex drivers are the real ones (conj is the identity, the rotation's cosine is real).  Same flag, count
    and resvec length; resvec and x within 1e-12 relative, the tolerance of the same pin for the cycle in tests/test_complex_host.py
    (measured: 1.5e-15 in resvec, 1.8e-14 in x)."""
    A, mesh = mg.poisson_shifted([8, 8, 8])
    pr = mg.getMGparam(np.float64, np.int64, 2, 8, 30, 1e-8, relax, 0.8, 2, 1, cyc, "NoMUMPS", 0.5, 0.0)
    pc = mg.getMGparam(np.complex128, np.int64, 2, 8, 30, 1e-8, relax, 0.8, 2, 1, cyc, "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(A, mesh, pr)
    mg.MGsetup(A, mesh, pc)
    b = mg.seeded_rhs(A)
    bc = b.astype(np.complex128)
    Ar = lambda v: A @ v
    runs = [(orc.bicgstb(Ar, b, 1e-8, 30, orc.getMultigridPreconditioner(pr, b), np.zeros_like(b)),
             ck.bicgstb(Ar, bc, 1e-8, 30, ck.preconditioner(pc), None))]
    for inner in (3, 5):
        runs.append((orc.fgmres(Ar, b, inner, 1e-8, 30, orc.getMultigridPreconditioner(pr, b), np.zeros_like(b)),
                     ck.fgmres(Ar, bc, inner, 1e-8, 30, ck.preconditioner(pc), None)))
    for (xr, fr, itr, rvr), (xc, fc, itc, rvc) in runs:
        assert (fr, itr, len(rvr)) == (fc, itc, len(rvc))
        assert fr in (0, -3) and itr > 1
        dr = np.abs(rvr - rvc).max() / rvr[0]
        dx = np.abs(xr - xc).max() / np.abs(xr).max()
        print(f"  resvec diff {dr:.2e}, x diff {dx:.2e}")
        assert dr <= 1e-12 and dx <= 1e-12


RUNS = [(c, "bicgstab", None) for c in ("C1", "C2", "C3")] + [("C1", "fgmres", 5), ("C1", "fgmres", 10), ("C2", "fgmres", 10),
                                                             ("C3", "fgmres", 5), ("C3", "fgmres", 10)]


@pytest.mark.parametrize("name,method,inner", RUNS)
def test_complex_oracle_converges_on_the_shared_cases(mg, name, method, inner):
    """The oracle solves A_sys x = b (k h = 0.5, system damping 0.05 / 0 / 0.05) to ||b - A x|| / ||b|| < 1e-8 preconditioned by one
    cycle of the hierarchy on the operator with damping 0.5.  Counts (ck.EXPECTED): C1 BiCGSTAB 19 iterations (flag -3), FGMRES(5) 57
    steps, FGMRES(10) 45; C2 BiCGSTAB 27 (flag 0), FGMRES(10) 67 (FGMRES(5) takes 98 of the 100 steps of 20 restarts: left out);
    C3 BiCGSTAB 11 (flag -3), FGMRES(5) 43, FGMRES(10) 22.  The entry that stops each run sits at least 4 % below tol and the one
    before it at least 1 % above (the closest: 1.6 %, C2 FGMRES(10), so 4 % cannot be asked of it): a perturbation of every product and cycle by 4e-16 relative
    moved the histories by at most 1.5e-12 relative, so the device's rounding cannot move a count."""
    p, As, b = ck.case(mg, name)
    x, flag, it, rv = ck.reference(mg, name, method, inner)
    print(f"  {name} {method} {inner}: flag {flag}, count {it}, last entries {rv[-2]:.3e} {rv[-1]:.3e}")
    assert np.linalg.norm(b - As @ x) / np.linalg.norm(b) < 1e-8
    if method == "bicgstab":
        assert (it, flag) == ck.EXPECTED[name]["bicgstab"]
        assert len(rv) == 2 * it + (0 if flag == -3 else 1)
    else:
        assert flag == 0 and it == ck.EXPECTED[name][inner] and len(rv) == it
    assert rv[-1] < 0.96 * ck.TOL and rv[-2] > 1.01 * ck.TOL


def test_python_layer_refusals(mg):
    A, mesh = mg.poisson_shifted([8, 8, 8])
    pr = mg.getMGparam(np.float64, np.int64, 2, 8, 6, 1e-8, "Jac", 0.8, 2, 1)
    pc = mg.getMGparam(np.complex128, np.int64, 2, 8, 6, 1e-8, "Jac", 0.8, 2, 1)
    mg.MGsetup(A, mesh, pr)
    mg.MGsetup(A, mesh, pc)
    n = A.shape[0]
    b, bc = np.ones(n), np.ones(n, dtype=np.complex128)
    with pytest.raises(TypeError, match="solveBiCGSTAB_MG"):                       # a real param: pointed to the unsuffixed function
        mg.solveBiCGSTAB_MG_CFP64(A, pr, b, np.zeros_like(b))
    with pytest.raises(TypeError, match="solveGMRES_MG"):
        mg.solveGMRES_MG_CFP64(A, pr, b, np.zeros_like(b), True, 5)
    B = np.ones((n, 2), dtype=np.complex128, order="F")                            # a block of right-hand sides
    with pytest.raises(NotImplementedError):
        mg.solveBiCGSTAB_MG_CFP64(None, pc, B, np.zeros_like(B))
    with pytest.raises(NotImplementedError):
        mg.solveGMRES_MG_CFP64(None, pc, B, np.zeros_like(B), True, 5)
    s = mg.getMGsolver(pc, mesh, 2, "PCG")                                          # PCG stays out of scope for complex values
    with pytest.raises(NotImplementedError):
        mg.solveLinearSystem_(pc.As[0], bc, np.zeros_like(bc), s)
