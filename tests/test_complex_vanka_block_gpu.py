"""-m gpu: blocks of right-hand sides on complex Vanka hierarchies (``getMGparam(..., complexVanka=True, vankaBlocks=True)``; the
handle's option vanka_blocks) - the block form of the smoother alone against the one-vector kernels bit for bit, the block cycle,
block solveMG and the block drivers against the column-wise restatement of tests/complex_vanka_block_cases.py, and the return
codes of the C ABI.

Bounds.  Smoother: np.array_equal - a lane owns one (row, column) sum and forms it by the expressions of the one-vector kernel.
ComplexF64 cycles: 1e-11 of max|x| per column, the TOL of tests/test_complex_vanka_gpu.py (the same kernels, the same sums).
ComplexF32: e_dev <= 4 e_ref with e_ref < 64 * 2^-24, as test_cf32_cycles there.  solveMG: the bounds of test_solve_mg_history
there.  Drivers: flag 0, true residual of every column <= 1e-6, block-FGMRES steps within 1 of the oracle's recorded count.  The
conditions on the inputs are tests/test_complex_vanka_block_host.py's."""
import ctypes as C

import numpy as np
import pytest
import torch

import complex_vanka_block_cases as BC
import complex_vanka_cases as CV
import vanka_cases as V

pytestmark = pytest.mark.gpu

TOL = 1e-11
MG_ERR_INVALID, MG_ERR_UNSUPPORTED = 1, 4
C64 = np.complex64
dp = C.POINTER(C.c_double)


def _dev_block(a):
    """A host block as the contiguous row-major device tensor the _dev entries take."""
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the smoother alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cx", [False, True], ids=["FP64", "CFP64"])
@pytest.mark.parametrize("vname", ["VankaFaces", "EconVankaFaces", "VankaFacesAdd"])
@pytest.mark.parametrize("n,ip", BC.SMOOTHER_SHAPES, ids=[f"{'x'.join(map(str, n))}{'m' if ip else 'f'}" for n, ip in BC.SMOOTHER_SHAPES])
def test_block_smoother_equals_the_columns(mg, built, n, ip, vname, cx):
    """mg_vanka_apply_block_* against k calls of mg_vanka_apply_* on the columns, for k = 1, 3, 16 and numit = 1, 2, from a random
    block x: equal bits.  Also: permuted columns give the permuted result, an all-zero column of b with zero x stays zero, two runs
    give equal bits, and the _dev form (row-major device blocks) equals the host form (column-major)."""
    vtype = CV.VTYPES[vname]
    A = V.mixed_operator(n, ip, omega=V.REF_OMEGA) if cx else V.mixed_operator(n, ip)
    nn = np.asarray(n)
    D = mg.setupVankaFacesPreconditioner(A, nn, 0.6, ip, vtype)
    N = A.shape[0]
    relax = lambda x, b, numit: mg.RelaxVankaFacesColor(A, x, b, D, numit, 1, nn, ip, vtype, handle=H)
    with mg.vanka.vanka_handle(A, D, nn, ip) as H:
        for k in BC.SMOOTHER_K:
            B = BC.block(N, k, seed=61, zero_col=1 if k > 1 else None, cx=cx)
            X0 = BC.block(N, k, seed=67, zero_col=1 if k > 1 else None, cx=cx)
            for numit in (1, 2):
                cols = [relax(X0[:, c].copy(), B[:, c].copy(), numit) for c in range(k)]
                Xb = relax(X0.copy(order="F"), B, numit)
                assert Xb.shape == (N, k) and not np.array_equal(Xb[:, 0], X0[:, 0])
                for c in range(k):
                    assert np.array_equal(Xb[:, c], cols[c]), f"k={k} numit={numit} column {c}"
                if k > 1:
                    assert not Xb[:, 1].any()
                assert np.array_equal(relax(X0.copy(order="F"), B, numit), Xb)                      # two runs
                perm = np.arange(k)[::-1]
                Xp = relax(np.asfortranarray(X0[:, perm]), np.asfortranarray(B[:, perm]), numit)
                assert np.array_equal(Xp, Xb[:, perm])
                Xc = relax(np.array(X0, order="C"), np.array(B, order="C"), numit)                  # a C-ordered host block (a copy)
                assert np.array_equal(Xc, Xb)
                Xt = H.apply_dev(_dev_block(X0), _dev_block(B), numit, vtype)
                assert np.array_equal(Xt.cpu().numpy(), Xb)
        # one column through the _dev vector form; the column limits of the C ABI, x untouched
        xt = H.apply_dev(_dev_block(X0[:, 0]), _dev_block(B[:, 0]), 2, vtype)
        assert np.array_equal(xt.cpu().numpy(), cols[0])
        lib = mg.device.load_library()
        apply = lib.mg_vanka_apply_block_CFP64 if cx else lib.mg_vanka_apply_block_FP64
        B17, X17 = BC.block(N, 17, seed=61, cx=cx), BC.block(N, 17, seed=67, cx=cx)
        keep = X17.copy()
        assert apply(H.h, X17.ctypes.data_as(dp), B17.ctypes.data_as(dp), 17, 1, vtype) == MG_ERR_UNSUPPORTED
        assert apply(H.h, X17.ctypes.data_as(dp), B17.ctypes.data_as(dp), 0, 1, vtype) == MG_ERR_INVALID
        assert apply(H.h, X17.ctypes.data_as(dp), B17.ctypes.data_as(dp), 2, 1, 4) == MG_ERR_UNSUPPORTED   # FULL_VANKA_LEX
        assert np.array_equal(X17, keep)


# ---- the block cycle, ComplexF64 ---------------------------------------------------------------------------------------------------
def _col_err(X, ref):
    """The largest per-column error, of max|x| of the column; an all-zero reference column must be zero."""
    e = 0.0
    for j in range(ref.shape[1]):
        if not ref[:, j].any():
            assert not X[:, j].any(), f"column {j} should have stayed zero"
        else:
            e = max(e, CV.err_max(X[:, j], ref[:, j]))
    return e


@pytest.mark.parametrize("k", [3, 16])
@pytest.mark.parametrize("cid", list(BC.BLOCK_CYCLES))
def test_block_cycle(mg, built, cid, k):
    """One cycle from zero and a second from the iterate, one all-zero column; block_cycle_dev gives block_cycle's bits; a
    single-vector cycle run before the block calls gives the same bits after them."""
    p, H, B, Xs, _ = BC.reference(mg, cid, k)
    b = np.array(B[:, 0])
    x_before = np.zeros_like(b)
    mg.recursiveCycle(p, b, x_before)
    X = np.zeros_like(B, order="F")
    mg.recursiveCycle(p, B, X)
    e1 = _col_err(X, Xs[0])
    X1 = X.copy()
    mg.recursiveCycle(p, B, X)
    e2 = _col_err(X, Xs[1])
    print(f"{cid} k={k}: first cycle {e1:.3e}, second cycle {e2:.3e} of max|x| per column")
    assert e1 <= TOL and e2 <= TOL
    dev = p.device
    Bt = _dev_block(B)
    Xt = torch.zeros_like(Bt)
    dev.block_cycle_dev(Bt, Xt, 1)
    torch.cuda.synchronize()
    assert np.array_equal(Xt.cpu().numpy(), X1)
    dev.block_cycle_dev(Bt, Xt, 0)
    torch.cuda.synchronize()
    assert np.array_equal(Xt.cpu().numpy(), X)
    Z = np.zeros_like(B, order="F")
    assert np.array_equal(mg.getMultigridPreconditioner(p, B)(B), X1)
    assert np.array_equal(dev.block_cycle(np.array(B, order="F"), Z, 1), X1)
    x_after = np.zeros_like(b)
    mg.recursiveCycle(p, b, x_after)
    assert np.array_equal(x_before, x_after) and CV.err_max(x_after, Xs[0][:, 0]) <= TOL


@pytest.mark.parametrize("relaxType", ["VankaFaces", "VankaFacesAdd"])
def test_from_zero_block_is_the_general_path_on_zero(mg, built, relaxType):
    """x_is_zero = 1 (the first pass of a level reads B and the blocks only) against x_is_zero = 0 on a zero block: the same bits."""
    p = BC.param(mg, "24v", relaxType=relaxType)
    B = BC.block(p.As[0].shape[0], 3, zero_col=1)
    mg.adjustMemoryForNumRHS(p, 1)
    dev = mg.to_device(p)
    runs = [dev.block_cycle(B, np.zeros_like(B, order="F"), z).copy() for z in (1, 0, 1, 0, -1)]
    assert runs[0].any() and np.all(np.isfinite(runs[0].view(np.float64)))
    for r in runs[1:]:
        assert np.array_equal(r, runs[0])
    H = CV.Hier(p)
    assert _col_err(runs[0], BC.restate_block_cycle(H, B, None, True, "V")) <= TOL


# ---- the block cycle, ComplexF32 ---------------------------------------------------------------------------------------------------
def test_cf32_block_cycle(mg, built):
    """mg_block_cycle_dev_CFP64 on a singlePrecision param: the mixed closure on the whole block, from zero."""
    p = BC.param(mg, "12v", single=True)
    Hs, Ho = CV.Hier(p), CV.Hier(p, widen=True)
    k = 3
    B = BC.block(p.As[0].shape[0], k)
    mg.adjustMemoryForNumRHS(p, 1)
    dev = mg.to_device(p)
    Bt = _dev_block(B)
    Xt = torch.full(Bt.shape, 1.0 + 1j, dtype=torch.complex128, device="cuda")
    dev.block_cycle_dev(Bt, Xt, 1)
    torch.cuda.synchronize()
    X = Xt.cpu().numpy()
    assert np.array_equal(mg.getMultigridPreconditioner(p, B)(B), X)
    for j in range(k):
        bs = B[:, j].astype(C64)
        xs = CV.restate_cycle(Hs, bs, None, True, "V")
        xo = CV.restate_cycle(Ho, bs.astype(np.complex128), None, True, "V")
        assert xs.dtype == C64 and xo.dtype == np.complex128
        e_ref, e_dev = CV.rel2(xs, xo), CV.rel2(X[:, j], xo)
        print(f"12v CF32 block column {j}: restatement {e_ref:.3e}, device {e_dev:.3e} from the complex128 cycle on the rounded hierarchy")
        assert e_ref < 64 * 2.0 ** -24
        assert e_dev <= 4 * e_ref


# ---- solveMG on a block ------------------------------------------------------------------------------------------------------------
def test_block_solve_mg_history(mg, built):
    p, H, B, Xs, res = BC.reference(mg, "24v", 3, cycles=5)
    assert p.maxOuterIter == 5 and p.relativeTol == 1e-30
    X = np.zeros_like(B, order="F")
    _, _, iters = mg.solveMG(p, B, X)
    e = np.abs(p.resvec - res).max() / res[0]
    ex = _col_err(X, Xs[-1])
    print(f"24v k=3: residual history {e:.3e} of resvec[0], X {ex:.3e} per column; factors {np.round(p.resvec[1:] / p.resvec[:-1], 3)}")
    assert iters == 5 and p.resvec.shape == res.shape
    assert np.all(np.abs(p.resvec - res) <= 1e-10 * res[0]) and ex <= TOL


# ---- the block drivers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("single", [False, True], ids=["CF64", "CF32"])
def test_block_drivers(mg, built, single):
    """Block FGMRES(5) and block BiCGSTAB on the lightly damped K, k = 3, tol 1e-8, preconditioned by one block cycle."""
    p, K, B = BC.driver_problem(mg, single)
    it_o = BC.DRIVER_STEPS[single]
    bn = np.linalg.norm(B, axis=0)
    X = np.zeros_like(B, order="F")
    _, _, it, resvec = mg.solveBlockGMRES_MG_CFP64(K, p, B, X, True, BC.DRIVER_INNER)
    r = np.linalg.norm(B - K @ X, axis=0) / bn
    print(f"block FGMRES(5) single={single}: {it} inner steps (oracle {it_o}), true residuals {r}")
    assert p.flag == 0 and abs(it - it_o) <= 1 and np.all(r <= 1e-6)
    Bt = _dev_block(B)
    Xt = torch.zeros_like(Bt)
    flag, itd, _ = p.device.block_fgmres_dev_CFP64(Bt, Xt, BC.DRIVER_INNER, BC.DRIVER_TOL, BC.DRIVER_MAXIT)
    torch.cuda.synchronize()
    assert flag == 0 and itd == it and np.array_equal(Xt.cpu().numpy(), X)
    X = np.zeros_like(B, order="F")
    _, _, itb, _ = mg.solveBlockBiCGSTAB_MG_CFP64(K, p, B, X)
    r = np.linalg.norm(B - K @ X, axis=0) / bn
    print(f"block BiCGSTAB single={single}: {itb} iterations, true residuals {r}")
    assert p.flag == 0 and np.all(r <= 1e-6)
    Xt = torch.zeros_like(Bt)
    flag, itd, _ = p.device.block_bicgstab_dev_CFP64(Bt, Xt, BC.DRIVER_TOL, BC.DRIVER_MAXIT)
    torch.cuda.synchronize()
    assert flag == 0 and itd == itb and np.array_equal(Xt.cpu().numpy(), X)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_cabi(mg, built):
    lib = mg.device.load_library()
    p, H, B, Xs, _ = BC.reference(mg, "24v", 3)
    n = B.shape[0]
    B = np.array(B, order="F")
    mark = np.full(B.shape, 3.0 - 2.0j, order="F")

    def block_cycle(h, Bb, X, k, z=1):
        return lib.mg_block_cycle_CF64(h, Bb.ctypes.data_as(dp), X.ctypes.data_as(dp), n, k, z)

    # option off (the handle's default, an unflagged param): refused as before, X untouched
    pu = BC.param(mg, "24v", flagged=False)
    mg.adjustMemoryForNumRHS(pu, 1)
    du = mg.to_device(pu)
    X = mark.copy(order="F")
    assert block_cycle(du.handle, B, X, 3) == MG_ERR_UNSUPPORTED and np.array_equal(X, mark)
    assert b"not served on a complex Vanka hierarchy" in lib.mg_last_error()
    # option on
    mg.adjustMemoryForNumRHS(p, 1)
    dev = mg.to_device(p)
    hd = dev.handle
    X1 = np.zeros_like(B, order="F")
    assert block_cycle(hd, B, X1, 3) == 0 and _col_err(X1, Xs[0]) <= TOL
    B17 = BC.block(n, 17)
    X17 = np.full(B17.shape, 3.0 - 2.0j, order="F")
    assert block_cycle(hd, B17, X17, 17) == MG_ERR_UNSUPPORTED and np.all(X17 == 3.0 - 2.0j)
    assert block_cycle(hd, B, X, 0) == MG_ERR_INVALID and np.array_equal(X, mark)
    assert lib.mg_set_vanka_relax_CF64(hd, ord("K")) == 0 and lib.mg_finalize(hd) == 0                 # the K schedule
    assert block_cycle(hd, B, X, 3) == MG_ERR_UNSUPPORTED and np.array_equal(X, mark)
    assert lib.mg_set_vanka_relax_CF64(hd, ord("V")) == 0 and lib.mg_finalize(hd) == 0
    assert lib.mg_set_option(hd, b"vanka_blocks", 0.0) == 0                                            # read at every call
    assert block_cycle(hd, B, X, 3) == MG_ERR_UNSUPPORTED and np.array_equal(X, mark)
    assert lib.mg_set_option(hd, b"vanka_blocks", 1.0) == 0
    X2 = np.zeros_like(B, order="F")
    assert block_cycle(hd, B, X2, 3) == 0 and np.array_equal(X2, X1)                                   # the handle still serves
    _, _, B16, Xs16, _ = BC.reference(mg, "24v", 16)                                                   # a wider block grows the work set
    X16 = np.zeros(B16.shape, dtype=np.complex128, order="F")
    assert block_cycle(hd, np.array(B16, order="F"), X16, 16) == 0 and _col_err(X16, Xs16[0]) <= TOL
    X3 = np.zeros_like(B, order="F")
    assert block_cycle(hd, B, X3, 3) == 0 and np.array_equal(X3, X1)
