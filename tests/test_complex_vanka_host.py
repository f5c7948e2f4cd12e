"""CPU side of the complex Vanka hierarchies (``getMGparam(np.complex128, ..., complexVanka=True)``): the flag's validation,
what MGsetup builds with it, the refusals that precede the device, and the condition on the inputs of the GPU tests - every
residual factor of each case's restatement (tests/complex_vanka_cases.py) below 0.5 over five cycles."""
import numpy as np
import pytest
import scipy.sparse as sp

import complex_vanka_cases as CV
import vanka_cases as V
from complex_kcycle_oracle import rn_clear_of_tol

MIXED = "SystemsFacesMixedLinear"


def _param(mg, relaxType="VankaFaces", w=0.6, levels=3, cycle="V", transfer=MIXED, VAL=np.complex128, **kw):
    return mg.getMGparam(VAL, np.int64, levels, 1, 5, 1e-8, relaxType, w, 1, 1, cycle, "NoMUMPS", 0.4, 0.0, transfer, **kw)


def test_flag_validation(mg):
    p = _param(mg, complexVanka=True)
    assert p.complexVanka is True and p.VAL == np.complex128
    assert _param(mg).complexVanka is False
    ps = _param(mg, complexVanka=True, singlePrecision=True)
    assert ps.complexVanka and ps.singlePrecision and ps.VAL == np.complex64
    for rt in ("EconVankaFaces", "VankaFacesAdd", "VankaFacesLex"):          # (Lex is a Vanka type: the device refuses it later)
        assert _param(mg, relaxType=rt, complexVanka=True).complexVanka
    with pytest.raises(NotImplementedError):
        _param(mg, VAL=np.float64, complexVanka=True)
    for rt in ("Jac", "SPAI", "Jac-GMRES"):
        with pytest.raises(NotImplementedError):
            _param(mg, relaxType=rt, complexVanka=True)
    with pytest.raises(TypeError):                                           # keyword only
        mg.getMGparam(np.complex128, np.int64, 3, 1, 5, 1e-8, "VankaFaces", 0.6, 1, 1, "V", "NoMUMPS", 0.4, 0.0, MIXED, True)
    for q in (p, ps):
        c = mg.copySolver(q)
        assert c.complexVanka and c.singlePrecision == q.singlePrecision and c.VAL == q.VAL and c.relaxType == q.relaxType
    assert not mg.copySolver(_param(mg)).complexVanka


@pytest.mark.parametrize("transfer,n", [(MIXED, [24, 16]), ("SystemsFacesLinear", [24, 16]), (MIXED, [12, 8, 10])])
def test_setup(mg, transfer, n):
    mixed = transfer == MIXED
    A = V.mixed_operator(n, mixed, omega=0.15)
    M = CV.mesh(mg, n)
    levels = 3 if len(n) == 2 else 2
    p = _param(mg, levels=levels, transfer=transfer, complexVanka=True)
    mg.MGsetup(A, M, p)
    pr = _param(mg, levels=levels, transfer=transfer, VAL=np.float64)
    mg.MGsetup(V.mixed_operator(n, mixed), M, pr)
    assert p.levels == levels == pr.levels and [m.n.tolist() for m in p.Meshes] == [m.n.tolist() for m in pr.Meshes]
    for l in range(levels - 1):
        for X, Y in ((p.Ps[l], pr.Ps[l]), (p.Rs[l], pr.Rs[l])):
            assert X.dtype == np.float64 and np.array_equal(X.indptr, Y.indptr) and np.array_equal(X.indices, Y.indices)
            assert np.array_equal(X.data, Y.data)
        D = mg.setupVankaFacesPreconditioner(p.As[l], p.Meshes[l], 0.6, mixed, 1)
        assert p.relaxPrecs[l].dtype == np.complex64 and np.array_equal(p.relaxPrecs[l], D)
    assert all(Al.dtype == np.complex128 for Al in p.As) and len(p.relaxPrecs) == levels - 1
    ref = (p.Rs[0] @ A @ p.Ps[0]).toarray()
    assert np.abs(p.As[1].toarray() - ref).max() <= 1e-13 * np.abs(ref).max()
    # singlePrecision on top: complex64 As, float32 Ps / Rs, blocks from the complex64 operator
    ps = _param(mg, levels=levels, transfer=transfer, complexVanka=True, singlePrecision=True)
    mg.MGsetup(A, M, ps)
    assert all(Al.dtype == np.complex64 for Al in ps.As)
    for l in range(levels - 1):
        assert ps.Ps[l].dtype == np.float32 and ps.Rs[l].dtype == np.float32
        assert np.array_equal(ps.Ps[l].data, p.Ps[l].data.astype(np.float32)) and np.array_equal(ps.Rs[l].data, p.Rs[l].data.astype(np.float32))
        D = mg.setupVankaFacesPreconditioner(ps.As[l], ps.Meshes[l], 0.6, mixed, 1)
        assert ps.relaxPrecs[l].dtype == np.complex64 and np.array_equal(ps.relaxPrecs[l], D)
    assert np.array_equal(ps.As[0].data, sp.csr_matrix(A).astype(np.complex64).data)
    ref32 = (ps.Rs[0] @ (ps.As[0] @ ps.Ps[0])).toarray()            # R*(A*P), formed and kept in single
    assert np.array_equal(ps.As[1].toarray(), ref32)
    assert np.abs(ps.As[1].toarray() - ref).max() <= 1e-5 * np.abs(ref).max()


def test_setup_relax_param_forms(mg):
    """relaxParam a float, a pair, or one per level, exactly as for real hierarchies; the other served types; replaceMatrixInHierarchy
    recomputes the blocks on the host."""
    n = [24, 16]
    A = CV.operator(n, 0.15)
    M = CV.mesh(mg, n)
    p = _param(mg, w=(0.7, 0.5), complexVanka=True)
    mg.MGsetup(A, M, p)
    for l in range(2):
        assert np.array_equal(p.relaxPrecs[l], mg.setupVankaFacesPreconditioner(p.As[l], p.Meshes[l], (0.7, 0.5), True, 1))
    p = _param(mg, w=[0.7, (0.6, 0.4), 0.5], complexVanka=True)
    mg.MGsetup(A, M, p)
    assert np.array_equal(p.relaxPrecs[0], mg.setupVankaFacesPreconditioner(p.As[0], p.Meshes[0], 0.7, True, 1))
    assert np.array_equal(p.relaxPrecs[1], mg.setupVankaFacesPreconditioner(p.As[1], p.Meshes[1], (0.6, 0.4), True, 1))
    for rt, vt in (("EconVankaFaces", 3), ("VankaFacesAdd", 5)):
        q = _param(mg, relaxType=rt, complexVanka=True)
        mg.MGsetup(A, M, q)
        assert np.array_equal(q.relaxPrecs[1], mg.setupVankaFacesPreconditioner(q.As[1], q.Meshes[1], 0.6, True, vt))
    A2 = sp.csr_matrix(A * (2.0 - 0.5j))
    mg.replaceMatrixInHierarchy(q, A2)
    assert q.device is None and np.array_equal(q.As[0].data, A2.data)
    assert np.array_equal(q.relaxPrecs[0], mg.setupVankaFacesPreconditioner(A2, q.Meshes[0], 0.6, True, 5))
    assert np.array_equal(q.relaxPrecs[1], mg.setupVankaFacesPreconditioner(q.As[1], q.Meshes[1], 0.6, True, 5))
    assert np.allclose(q.As[1].toarray(), (q.Rs[0] @ A2 @ q.Ps[0]).toarray(), rtol=1e-13, atol=1e-13)


def test_refusals_precede_the_device(mg, monkeypatch):
    n = [16, 16]
    A = CV.operator(n, 0.15)
    M = CV.mesh(mg, n)
    N = A.shape[0]

    def no_device(*a, **k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(mg.device, "load_library", no_device)
    with pytest.raises(NotImplementedError):                                  # a default complex Vanka param is still refused
        mg.MGsetup(A, M, _param(mg, levels=2))
    with pytest.raises(NotImplementedError):
        mg.MGsetup(A, M, _param(mg, levels=2, singlePrecision=True))
    with pytest.raises(NotImplementedError):                                  # not a Systems transfer
        mg.MGsetup(A, M, _param(mg, levels=2, transfer="FullWeighting", complexVanka=True))
    b = CV.rhs(N)
    x = np.zeros_like(b)
    B = np.asfortranarray(np.stack([b, 2 * b], axis=1))
    X = np.zeros_like(B, order="F")
    for single in (False, True):
        p = _param(mg, levels=2, complexVanka=True, singlePrecision=single)
        mg.MGsetup(A, M, p)
        bb, xx = (b.astype(np.complex64), x.astype(np.complex64)) if single else (b, x)
        # blocks of more than one column, through every public route
        for call in (lambda: mg.solveMG(p, B, X), lambda: mg.recursiveCycle(p, B, X), lambda: mg.getMultigridPreconditioner(p, B),
                     lambda: mg.SpMatMul(p, 1, "A", B, X), lambda: mg.solveBlockBiCGSTAB_MG_CFP64(p.As[0], p, B, X),
                     lambda: mg.solveBlockGMRES_MG_CFP64(p.As[0], p, B, X, True, 5)):
            with pytest.raises(NotImplementedError):
                call()
        with pytest.raises(NotImplementedError):
            mg.transposeHierarchy(p)
        with pytest.raises(NotImplementedError):
            mg.adjointHierarchy(p)
        assert p.doTranspose == 0
        # the sharded forms
        from multigrid_jl_amd.distributed import DistributedHierarchy
        from multigrid_jl_amd.ghost_dist import ghost_gmg
        with pytest.raises(NotImplementedError):
            DistributedHierarchy.check_supported(p)
        with pytest.raises(NotImplementedError):
            DistributedHierarchy.check_supported(p, native=True)
        with pytest.raises(NotImplementedError):
            ghost_gmg(n, [1, 1], 0, 1, p, lambda m: None)
        # VankaFacesLex stays refused; ComplexF32 with 'K'
        bad = [_param(mg, relaxType="VankaFacesLex", levels=2, complexVanka=True, singlePrecision=single)]
        if single:
            bad.append(_param(mg, cycle="K", levels=2, complexVanka=True, singlePrecision=True))
        for q in bad:
            mg.MGsetup(A, M, q)
            with pytest.raises(NotImplementedError):
                mg.solveMG(q, bb, xx.copy())
            with pytest.raises(NotImplementedError):
                mg.solveGMRES_MG_CFP64(q.As[0], q, b, x.copy(), True, 5)
        # a Schwarz coarsest solve
        q = _param(mg, levels=2, complexVanka=True, singlePrecision=single)
        mg.MGsetup(A, M, q)
        q.LU = mg.getDomainDecompositionParam(np.complex128, np.int64, q.Meshes[-1], [2, 2], [1, 1])
        with pytest.raises(NotImplementedError):
            mg.recursiveCycle(q, bb, xx.copy())
        q.LU = None
        # a hierarchy whose flag was dropped by hand does not reach the device either
        q = _param(mg, levels=2, complexVanka=True, singlePrecision=single)
        mg.MGsetup(A, M, q)
        q.complexVanka = False
        with pytest.raises(NotImplementedError):
            mg.recursiveCycle(q, bb, xx.copy())


class _FakeLib:
    """Stands in for the library where a test needs a handle that exists: every entry point succeeds and is counted."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a):
            self.calls.append(name)
            return 0
        return fn


def test_relax_type_switch_after_upload_raises(mg, monkeypatch):
    """relaxType switched to or from Vanka after the upload: refused by sync_schedule before anything is sent."""
    n = [16, 16]
    A = CV.operator(n, 0.15)
    for single in (False, True):
        p = _param(mg, levels=2, complexVanka=True, singlePrecision=single)
        mg.MGsetup(A, CV.mesh(mg, n), p)
        fake = _FakeLib()
        monkeypatch.setattr(mg.device, "load_library", lambda *a, **k: fake)
        dev = mg.to_device(p)
        try:
            assert f"mg_set_vanka_{'CF32' if single else 'CF64'}" in fake.calls and f"mg_set_vanka_relax_{'CF32' if single else 'CF64'}" in fake.calls
            assert "mg_set_schedule_CF64" not in fake.calls and "mg_set_relax_type" not in fake.calls
            sent = len(fake.calls)
            for rt in ("Jac", "EconVankaFaces"):
                p.relaxType = rt
                with pytest.raises(NotImplementedError):
                    mg.to_device(p)
                assert len(fake.calls) == sent
            p.relaxType = "VankaFaces"
            p.cycleType = "W"                                                 # a served change goes through the Vanka setter
            mg.to_device(p)
            assert fake.calls[sent:].count(f"mg_set_vanka_relax_{'CF32' if single else 'CF64'}") == 1 and fake.calls[-1] == "mg_finalize"
            # and a pointwise complex hierarchy cannot be switched to Vanka
        finally:
            dev.handle = None
            p.device = None
        pj = _param(mg, relaxType="Jac", levels=2, transfer=MIXED, singlePrecision=single)
        mg.MGsetup(A, CV.mesh(mg, n), pj)
        dev = mg.to_device(pj)
        try:
            pj.relaxType, pj.complexVanka = "VankaFaces", True
            with pytest.raises(NotImplementedError):
                mg.to_device(pj)
        finally:
            dev.handle = None
            pj.device = None


@pytest.mark.parametrize("name", list(CV.CASES))
def test_restatement_contracts(mg, name):
    """The condition on the input (CPU arithmetic only): every residual factor of the restatement's five cycles is below 0.5.
    K case: no residual estimate of a K step lies within a factor 4 of the break's 1e-5 (they lie between 0.009 and 1.3)."""
    p, H, b, xs, res, trace = CV.reference(mg, name, cycles=5)
    f = res[1:] / res[:-1]
    print(name, "factors", np.round(f, 3))
    assert f.shape == (5,) and np.all(f < 0.5)
    if p.cycleType == "K":
        rn = np.array([r for rec in trace for r in rec[4]])
        print(name, "K-step residual estimates", rn.min(), rn.max())
        assert len(trace) == 5 and all(rec[3] == 2 for rec in trace) and rn_clear_of_tol(trace)
    else:
        assert trace == []


def test_restatement_is_the_vanka_cases_vcycle(mg):
    """The recursion written once more in complex_vanka_cases gives the bits of vanka_cases.restate_vcycle for V and W, in
    complex128 and in complex64."""
    for name in ("24v", "24w"):
        for single in (False, True):
            p = CV.param(mg, name, single=single)
            H = CV.Hier(p)
            b = CV.rhs(p.As[0].shape[0], single)
            cyc = p.cycleType
            c1 = CV.restate_cycle(H, b, None, True, cyc)
            c2 = CV.restate_cycle(H, b, c1, False, cyc)
            v1 = V.restate_vcycle(H.As, H.Ps, H.Rs, H.Ds, H.ns, True, V.FULL_VANKA_RB, H.lu, b, None, True, 1, 1, cyc)
            v2 = V.restate_vcycle(H.As, H.Ps, H.Rs, H.Ds, H.ns, True, V.FULL_VANKA_RB, H.lu, b, v1.copy(), False, 1, 1, cyc)
            assert c1.dtype == b.dtype and np.array_equal(c1, v1) and np.array_equal(c2, v2)
