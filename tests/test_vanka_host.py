"""Host mirror of src/Multigrid/Vanka.jl and Systems.jl (no GPU): index lists, colouring, block setup, the 1-D and Kronecker
transfer operators, MGsetup with the Systems operators, and every combination that must keep raising."""
import numpy as np
import pytest
import scipy.sparse as sp

import vanka_cases as V


# ---- index lists and colours ---------------------------------------------------------------------------------------------
def _brute_force(n, ip):
    """The unknowns of every cell from the face ARRAYS themselves: number them in the stated order, read each cell's faces."""
    dim = len(n)
    off = 0
    arrays = []
    for j in range(dim):
        shape = [n[k] + (1 if k == j else 0) for k in range(dim)]
        size = int(np.prod(shape))
        arrays.append(np.arange(off + 1, off + size + 1).reshape(shape, order="F"))
        off += size
    P = np.arange(off + 1, off + int(np.prod(n)) + 1).reshape(n, order="F")
    out = []
    for cell in np.ndindex(*n[::-1]):
        c = cell[::-1]
        I = []
        for j in range(dim):
            lo, hi = list(c), list(c)
            hi[j] += 1
            I += [arrays[j][tuple(lo)], arrays[j][tuple(hi)]]
        if ip:
            I.append(P[tuple(c)])
        out.append(I)
    return np.array(out)


@pytest.mark.parametrize("n", [[3, 4], [4, 3, 5]])
@pytest.mark.parametrize("ip", [False, True])
def test_index_lists(mg, n, ip):
    bs, nf = mg.getVankaBlockSize(np.asarray(n), ip)
    assert bs == 2 * len(n) + int(ip)
    ref = _brute_force(n, ip)
    for ii in range(1, int(np.prod(n)) + 1):
        I = mg.getVankaVariablesOfCell(mg.cs2loc(ii, n), n, nf, np.zeros(bs, dtype=np.int64), ip)
        assert np.array_equal(I, ref[ii - 1]) and np.all(np.diff(I) > 0)
    assert np.array_equal(mg.vanka._all_cell_indices(np.asarray(n), nf, ip), ref)
    assert np.array_equal(V.all_unknowns(n, ip), ref)


@pytest.mark.parametrize("n", [[3, 4], [4, 3, 5]])
def test_colours(mg, n):
    ref = _brute_force(n, True)
    cols = np.array([mg.cellColor(mg.cs2loc(ii, n)) for ii in range(1, int(np.prod(n)) + 1)])
    assert sorted(set(cols)) == list(range(1, 2 ** len(n) + 1))
    for c in set(cols):
        members = ref[cols == c].ravel()
        assert len(set(members)) == members.size              # no two cells of a class share an unknown
    assert mg.cellRBColor([1, 1]) == 1 and mg.cellRBColor([1, 2]) == 2 and mg.cellRBColor([2, 2, 1]) == 2


def test_types_and_constants(mg):
    assert (mg.FULL_VANKA_RB, mg.KACMARZ_VANKA, mg.ECON_VANKA_RB, mg.FULL_VANKA_LEX, mg.FULL_VANKA_ADD) == (1, 2, 3, 4, 5)
    assert mg.getVankaRelaxType("VankaFaces") == (True, 1) and mg.getVankaRelaxType("EconVankaFaces") == (True, 3)
    assert mg.getVankaRelaxType("VankaFacesLex") == (True, 4) and mg.getVankaRelaxType("VankaFacesAdd") == (True, 5)
    assert mg.getVankaRelaxType("Jac") == (False, 0)


# ---- block setup -----------------------------------------------------------------------------------------------------------
def _expected_block(Acc, vtype, w, ip, loc, n):
    bs = Acc.shape[0]
    Acc = Acc.copy()
    scalar = not isinstance(w, tuple)
    W = np.full(bs, w if scalar else w[0], dtype=float)
    if not scalar and ip:
        W[-1] = w[1]
    if vtype in (1, 4):
        if scalar:
            Acc[:-1, :-1] = np.diag(np.diag(Acc[:-1, :-1]))
            Minv = w * np.linalg.inv(Acc)
        else:
            Minv = W[:, None] * np.linalg.inv(Acc)
    elif vtype == 3:
        Acc[:-1, :-1] = np.diag(np.diag(Acc[:-1, :-1]) / w)
        Minv = np.linalg.inv(Acc)
    else:
        t = np.full(bs, 0.5)
        for d in range(len(n)):
            if loc[d] == 1:
                t[2 * d] = 1.0
            if loc[d] == n[d]:
                t[2 * d + 1] = 1.0
        if ip:
            t[-1] = 1.0
        Minv = (t * W)[:, None] * np.linalg.inv(Acc)
    return Minv.conj().T.ravel(order="F")          # AccInv = (.)' flattened column-major


@pytest.mark.parametrize("n,ip", [([3, 4], True), ([3, 4], False), ([4, 3, 5], True)])
@pytest.mark.parametrize("cx", [False, True])
@pytest.mark.parametrize("vtype,w", [(1, 0.6), (1, (0.7, 0.5)), (4, 0.6), (3, 0.8), (5, 0.6), (5, (0.7, 0.5))])
def test_block_setup(mg, n, ip, cx, vtype, w):
    A = V.mixed_operator(n, ip, omega=0.8 if cx else None)
    D = mg.setupVankaFacesPreconditioner(A, mg.getRegularMesh([0, 1] * len(n), n), w, ip, vtype)
    bs = 2 * len(n) + int(ip)
    assert D.shape == (bs * bs, int(np.prod(n))) and D.dtype == (np.complex64 if cx else np.float32) and D.flags.f_contiguous
    ref = _brute_force(n, ip) - 1
    Ad = A.toarray()
    for c in range(D.shape[1]):
        I = ref[c]
        want = _expected_block(Ad[np.ix_(I, I)], vtype, w, ip, mg.cs2loc(c + 1, n), n)
        assert np.array_equal(D[:, c], want.astype(D.dtype)) or np.allclose(D[:, c], want, rtol=2e-6, atol=0)
        # the adjoint layout: reshape(D[:, c], bs, bs)' applied to r is the damped inverse applied to r
        M = D[:, c].reshape(bs, bs, order="F").conj().T
        assert np.allclose(M, want.reshape(bs, bs, order="F").conj().T, rtol=2e-6)


def test_scalar_w_is_the_economic_variant(mg):
    """FULL_VANKA_RB with a scalar w drops the off-diagonal face couplings before inverting (Vanka.jl:333): it differs from the
    full inverse and equals ECON's block up to where w enters."""
    n = [3, 4]
    A = V.mixed_operator(n, True)
    D = mg.setupVankaFacesPreconditioner(A, np.asarray(n), 0.6, True, mg.FULL_VANKA_RB)
    I = _brute_force(n, True)[5] - 1
    Acc = A.toarray()[np.ix_(I, I)]
    full = (0.6 * np.linalg.inv(Acc)).T.ravel(order="F").astype(np.float32)
    econ = Acc.copy()
    econ[:-1, :-1] = np.diag(np.diag(econ[:-1, :-1]))
    assert np.abs(Acc[:-1, :-1] - econ[:-1, :-1]).max() > 0
    assert not np.allclose(D[:, 5], full, rtol=1e-3)
    assert np.allclose(D[:, 5], (0.6 * np.linalg.inv(econ)).T.ravel(order="F"), rtol=2e-6)


# ---- the 1-D Systems operators at n = 8, entry by entry --------------------------------------------------------------------
def test_1d_operators_at_8(mg):
    R, nc = mg.get1DNodeInjection(8)
    want = np.zeros((5, 9))
    want[np.arange(5), 2 * np.arange(5)] = 1.0
    assert nc == 4 and np.array_equal(R.toarray(), want)

    R, nc = mg.get1DNodeFullWeightRestriction(8)
    want = np.array([[1, .5, 0, 0, 0, 0, 0, 0, 0],
                     [0, .5, 1, .5, 0, 0, 0, 0, 0],
                     [0, 0, 0, .5, 1, .5, 0, 0, 0],
                     [0, 0, 0, 0, 0, .5, 1, .5, 0],
                     [0, 0, 0, 0, 0, 0, 0, .5, 1]])
    assert nc == 4 and np.array_equal(R.toarray(), want)

    # Julia's spdiagm gives the main diagonal n-1 entries, so (8, 8) of the banded matrix is zero - in a column that the
    # selection 1:2:end drops; P[1, 1] = 1 and P[end, end] = 1 overwrite two .75s (the last one in Julia's column 7)
    P, nc = mg.get1DProlongationCellCentered(8)
    want = np.array([[1, 0, 0, 0],
                     [.75, .25, 0, 0],
                     [.25, .75, 0, 0],
                     [0, .75, .25, 0],
                     [0, .25, .75, 0],
                     [0, 0, .75, .25],
                     [0, 0, .25, .75],
                     [0, 0, 0, 1]])
    assert nc == 4 and np.array_equal(P.toarray(), want)

    R, nc = mg.systems.get1DRestrictionCells(8)
    want = np.zeros((4, 8))
    want[np.arange(4), 2 * np.arange(4)] = 1.0
    want[np.arange(4), 2 * np.arange(4) + 1] = 1.0
    assert nc == 4 and np.array_equal(R.toarray(), want)

    P, nc = mg.get1DProlongationNodes(8)
    want = np.zeros((9, 5))
    for j in range(5):
        want[2 * j, j] = 1.0
        if j > 0:
            want[2 * j - 1, j] = .5
        if j < 4:
            want[2 * j + 1, j] = .5
    assert nc == 4 and np.array_equal(P.toarray(), want)


def test_1d_operators_identity_below_8_and_odd_sizes(mg):
    S = mg.systems
    for k in (1, 4, 7):
        for f, m in ((S.get1DNodeInjection, k + 1), (S.get1DNodeFullWeightRestriction, k + 1), (S.get1DProlongationCellCentered, k),
                     (S.get1DRestrictionCells, k), (S.get1DProlongationNodes, k + 1)):
            M, nc = f(k)
            assert nc == k and np.array_equal(M.toarray(), np.eye(m))
    for f in (S.get1DNodeInjection, S.get1DNodeFullWeightRestriction, S.get1DProlongationCellCentered, S.get1DRestrictionCells,
              S.get1DProlongationNodes):
        with pytest.raises(ValueError):
            f(9)


@pytest.mark.parametrize("n", [[8, 12], [8, 4, 10]])
@pytest.mark.parametrize("mixed", [False, True])
def test_kronecker_shapes(mg, n, mixed):
    S = mg.systems
    P, R, nc = mg.getLinearOperatorsSystemsFaces(n, mixed)
    ncw = [k // 2 if k >= 8 else k for k in n]
    assert list(nc) == ncw
    count = lambda m: sum(int(np.prod([m[k] + (1 if k == j else 0) for k in range(len(m))])) for j in range(len(m))) \
        + (int(np.prod(m)) if mixed else 0)
    assert P.shape == (count(n), count(ncw)) and R.shape == (count(ncw), count(n))
    Rinj = mg.getInjectionOperatorsSystemsFaces(n, mixed)
    assert Rinj.shape == R.shape
    # the first block is kron(cells..., nodes) with the nodal operator in dimension 1
    ops = [S.get1DProlongationNodes(n[0])[0]] + [S.get1DProlongationCellCentered(k)[0] for k in n[1:]]
    K = ops[0]
    for M in ops[1:]:
        K = sp.kron(M, K)
    P1, _ = mg.getLinearInterpolationFacesUj(n, 1)
    assert (P1 != sp.csr_matrix(K)).nnz == 0 and (P[:P1.shape[0], :P1.shape[1]] != P1).nnz == 0
    # constants are interpolated exactly away from the corners' overwritten entries, and restricted with weight 2^dim
    Pc, _ = mg.getLinearInterpolationCellCentered(n)
    assert np.allclose(Pc @ np.ones(Pc.shape[1]), 1.0)
    Rc, _ = mg.getRestrictionCellCentered(n)            # the package's export; Systems.jl's is the same operator
    assert (sp.csr_matrix(Rc) != S.getRestrictionCellCentered(n)[0]).nnz == 0
    assert np.allclose(Rc @ np.ones(Rc.shape[1]), 2.0 ** sum(k >= 8 for k in n))


def _param(mg, relaxType="VankaFaces", w=0.6, levels=5, cycle="V", transfer="SystemsFacesMixedLinear", VAL=np.float64, coarse="NoMUMPS"):
    return mg.getMGparam(VAL, np.int64, levels, 1, 5, 1e-8, relaxType, w, 1, 1, cycle, coarse, 0.4, 0.0, transfer)


def test_mgsetup_mixed_32(mg):
    n = [32, 32]
    A = V.mixed_operator(n, True)
    # five levels asked for: 8 cells still coarsen (the 1-D operators are the identity BELOW 8), 4 do not - P is square there
    # and the setup stops with four levels (MGsetup.jl:84-92)
    p5 = _param(mg, levels=5)
    mg.MGsetup(A, mg.getRegularMesh([0, 1, 0, 1], n), p5)
    assert p5.levels == 4 and [m.n.tolist() for m in p5.Meshes] == [[32, 32], [16, 16], [8, 8], [4, 4]]
    assert len(p5.As) == 4 and len(p5.Ps) == 3 and len(p5.relaxPrecs) == 4 and p5.relaxPrecs[3].shape == (25, 16)
    p = _param(mg, levels=3)
    mg.MGsetup(A, mg.getRegularMesh([0, 1, 0, 1], n), p)
    assert p.levels == 3 and [m.n.tolist() for m in p.Meshes] == [[32, 32], [16, 16], [8, 8]]
    assert len(p.Ps) == 2 and len(p.relaxPrecs) == 2 and p.relaxPrecs[0].shape == (25, 1024) and p.relaxPrecs[1].shape == (25, 256)
    P, R, _ = mg.getLinearOperatorsSystemsFaces(n, True)
    assert (p.Ps[0] != P).nnz == 0 and np.array_equal(p.Rs[0].toarray(), 0.25 * R.toarray())      # RT scaled by 0.5^dim
    assert np.allclose(p.As[1].toarray(), (p.Rs[0] @ A @ p.Ps[0]).toarray(), rtol=1e-13, atol=1e-13)
    # faces only, and a tuple of two per level
    p2 = _param(mg, w=(0.7, 0.5), transfer="SystemsFacesLinear", levels=2)
    A2 = V.mixed_operator(n, False)
    mg.MGsetup(A2, mg.getRegularMesh([0, 1, 0, 1], n), p2)
    assert p2.levels == 2 and p2.relaxPrecs[0].shape == (16, 1024)
    assert np.array_equal(p2.relaxPrecs[0], mg.setupVankaFacesPreconditioner(A2, np.asarray(n), (0.7, 0.5), False, 1))
    # one entry per level: floats, pairs, in a tuple or a list
    for per_level in (((0.7, 0.5), (0.6, 0.4)), [(0.7, 0.5), (0.6, 0.4)], (0.7, 0.6)):
        p4 = _param(mg, w=per_level, transfer="SystemsFacesLinear", levels=2)
        if per_level == (0.7, 0.6):          # a pair of numbers is ONE (w1, w2), copied to every level
            mg.MGsetup(A2, mg.getRegularMesh([0, 1, 0, 1], n), p4)
            assert np.array_equal(p4.relaxPrecs[0], mg.setupVankaFacesPreconditioner(A2, np.asarray(n), (0.7, 0.6), False, 1))
            continue
        mg.MGsetup(A2, mg.getRegularMesh([0, 1, 0, 1], n), p4)
        assert np.array_equal(p4.relaxPrecs[0], mg.setupVankaFacesPreconditioner(A2, np.asarray(n), (0.7, 0.5), False, 1))
    # the Systems operators are built whatever the relaxType is
    p3 = _param(mg, relaxType="Jac", w=0.8, transfer="SystemsFacesLinear", levels=2)
    mg.MGsetup(A2, mg.getRegularMesh([0, 1, 0, 1], n), p3)
    assert p3.relaxPrecs[0].shape == (A2.shape[0],) and (p3.Ps[0] != p2.Ps[0]).nnz == 0
    # getRelaxPrec: the trailing arguments, and replaceMatrixInHierarchy passes them on
    D = mg.getRelaxPrec(A, "EconVankaFaces", 0.8, p.Meshes[0], True)
    assert np.array_equal(D, mg.setupVankaFacesPreconditioner(A, p.Meshes[0], 0.8, True, 3))
    mg.replaceMatrixInHierarchy(p, 2.0 * A)
    assert np.allclose(p.relaxPrecs[0], 0.5 * mg.setupVankaFacesPreconditioner(A, p.Meshes[0], 0.6, True, 1), rtol=1e-6)


def test_out_of_scope_raises(mg, monkeypatch):
    n = [8, 8]
    A = V.mixed_operator(n, True)
    M = mg.getRegularMesh([0, 1, 0, 1], n)
    N = A.shape[0]
    D = mg.setupVankaFacesPreconditioner(A, M, 0.6, True)

    def no_device(*a, **k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(mg.device, "load_library", no_device)
    x, b = np.zeros(N), np.ones(N)
    with pytest.raises(NotImplementedError):
        mg.setupVankaFacesPreconditioner(A, M, 0.6, True, mg.KACMARZ_VANKA)
    with pytest.raises(NotImplementedError):
        mg.RelaxVankaFacesColor(A, x, b, D, 1, 1, M, True, mg.FULL_VANKA_LEX)
    with pytest.raises(TypeError):
        mg.RelaxVankaFacesColor(A, x, b, D.astype(np.float64), 1, 1, M, True)              # "check types."
    with pytest.raises(TypeError):
        mg.RelaxVankaFacesColor(A, x, b, D.astype(np.complex64), 1, 1, M, True)
    with pytest.raises(TypeError):
        mg.RelaxVankaFacesColor(A, x.astype(np.complex128), b, D.astype(np.complex64), 1, 1, M, True)   # complex x, real operator
    with pytest.raises(ValueError):
        mg.RelaxVankaFacesColor(A, np.zeros(N - 1), b[:-1], D, 1, 1, M, True)
    with pytest.raises(ValueError):
        mg.RelaxVankaFacesColor(A, x, b, D, 1, 1, M, False)                                # length is not sum(nf)
    with pytest.raises(NotImplementedError):
        mg.MGsetup(A, M, _param(mg, coarse="VankaFaces"))
    with pytest.raises(NotImplementedError):
        mg.MGsetup(A.astype(np.complex128), M, _param(mg, VAL=np.complex128))              # complex Vanka hierarchies
    with pytest.raises(NotImplementedError):
        mg.MGsetup(A, M, _param(mg, transfer="SomethingElse"))
    with pytest.raises(NotImplementedError):
        mg.SA_AMGsetup(A, _param(mg, transfer="FullWeighting"))
    with pytest.raises(NotImplementedError):
        mg.getRelaxPrec(A, "hybridVankaFacesKaczmarz", 0.6, M, True)
    p = _param(mg, levels=2)
    mg.MGsetup(V.mixed_operator([16, 16], True), mg.getRegularMesh([0, 1, 0, 1], [16, 16]), p)
    with pytest.raises(NotImplementedError):
        mg.transposeHierarchy(p)
    b16 = np.ones(p.As[0].shape[0])
    for bad in (_param(mg, relaxType="VankaFacesLex", levels=2), _param(mg, cycle="K", levels=2)):
        mg.MGsetup(p.As[0], p.Meshes[0], bad)
        with pytest.raises(NotImplementedError):
            mg.solveMG(bad, b16, np.zeros_like(b16))
    B = np.ones((b16.size, 2), order="F")
    with pytest.raises(NotImplementedError):
        mg.solveMG(p, B, np.zeros_like(B, order="F"))
