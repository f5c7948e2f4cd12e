"""-m gpu: mg_rap_FP64 / _CF64 / _CF32 on the crafted hierarchy of tests/rap_crafted_cases.py - every entry of both refreshed coarse
operators against the long-double sum of its terms (formed from the finer level's values as read back from the device) within
the derived entry bound, every relaxation vector bit for bit against the documented expression; the shapes, the bounds and their
derivation are in that module's docstring, the wrong variants the checks catch in tests/test_rap_crafted_host.py.

A case is (value type, rap_chunk, rap_groups), set through the handle's options: chunks 1, 10, 2048 and 5000 (5000 must give the
bits of 2048; for float64 every chunk gives the same bits, the order of an entry's sum does not depend on it); the complex types
also with 1, 2, 8 and 16 lane groups.  Per case, on one resident handle: the coarse operators are overwritten with NaN
(replace_values), then refreshed - the crafted family with Jac and with SPAI vectors, once more (the same bits), the exact family
(bit-equal to the exact product on both levels).  The rows of R and A stored out of order are uploaded as they are: the upload
accepts them.

The unsorted coarse row (test_an_unsorted_coarse_row_is_refused_*): rap_numeric and cx_rap_numeric find a target column by binary
search in C's stored row, so a coarse operator with two columns of one row swapped would lose contributions silently; the upload
records it and mg_rap_* return MG_ERR_UNSUPPORTED before anything is written - the values and relaxation vectors stay bit for bit -
and mg.replaceMatrixInHierarchy takes the host path.  Operators with 64-bit row pointers are refused alike (one assertion below)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import rap_crafted_cases as K

pytestmark = pytest.mark.gpu

MG_ERR_UNSUPPORTED = 4
CHUNKS = (1, 10, 2048, 5000)
CASES = [("float64", c, 0) for c in CHUNKS] + [(vt, c, g) for vt in ("complex128", "complex64") for c in CHUNKS for g in (1, 2, 8, 16)]
SHARES = {}          # (value type, level) -> the largest share of a bound used so far (printed per case)
_REFS = {}
_BITS = {}
_CHECKED = set()


def _param(mg, vt, relax="Jac"):
    H, v = K.hierarchy(), K.values(vt, "crafted")
    kw = dict(singlePrecision=True, singleDeviceSetup=True) if vt == "complex64" else {}
    p = mg.getMGparam(np.float64 if vt == "float64" else np.complex128, np.int64, 3, 8, 1, 0.0, relax, K.OMEGA, 1, 1, "V",
                      "NoMUMPS", 0.5, 0.0, **kw)
    p.As = [H["A"][0].csr(v["A"]), H["C"][0].csr(K.initial_coarse(vt, 2)), H["C"][1].csr(K.initial_coarse(vt, 3))]
    p.Ps = [H["P"][l].csr(v["P"][l]) for l in (0, 1)]
    p.Rs = [H["R"][l].csr(v["R"][l]) for l in (0, 1)]
    rng = np.random.default_rng(5)
    p.relaxPrecs = [(rng.standard_normal(n) + (1j * rng.standard_normal(n) if vt != "float64" else 0)).astype(np.dtype(vt))
                    for n in (K.N1, K.N2)]
    S = sp.identity(K.N3) * (4.0 + (1j if vt != "float64" else 0)) + 0.1 * sp.random(K.N3, K.N3, density=0.2, random_state=5)
    p.LU = spla.splu(sp.csc_matrix(S))      # (the coarsest solve is never applied here; the upload needs one)
    p.nrhs = 1
    p.Meshes = []
    return p


def _rap_status(dev, vt, a1, kind):
    """mg_rap_* through the C ABI with new fine values (stored order, as applied); the status."""
    om = np.full(3, K.OMEGA)
    done = C.c_longlong(0)
    if vt == "float64":
        nz = np.ascontiguousarray(a1, dtype=np.float64)
        return dev.lib.mg_rap_FP64(dev.handle, nz.ctypes.data_as(C.POINTER(C.c_double)), nz.size, kind,
                                   om.ctypes.data_as(C.POINTER(C.c_double)), C.byref(done))
    nz = np.ascontiguousarray(np.conj(a1), dtype=np.dtype(vt))          # the reference's AT values
    return dev._fn("rap")(dev.handle, dev._vp_of(nz), nz.size, kind, om.ctypes.data_as(C.POINTER(C.c_double)), C.byref(done))


def _relax(dev, vt, level, n):
    from multigrid_jl_amd import device as D
    d = np.full(n, np.nan, dtype=np.dtype(vt))
    if vt == "float64":
        D._check(dev.lib, dev.lib.mg_get_relax_FP64(dev.handle, level, D._f64(d), n), "mg_get_relax")
    else:
        D._check(dev.lib, dev._fn("get_relax")(dev.handle, level, dev._vp_of(d), n), "mg_get_relax")
    return d


def _state(dev, vt):
    """What the re-setup writes, read back: As[2], As[3], relaxPrecs[1], relaxPrecs[2]."""
    from multigrid_jl_amd import device as D
    return ([np.asarray(dev.get_values(l, D.MG_OP_A)).astype(np.dtype(vt), copy=False) for l in (2, 3)],
            [_relax(dev, vt, 1, K.N1), _relax(dev, vt, 2, K.N2)])


def _poison(dev, vt):
    from multigrid_jl_amd import device as D
    H = K.hierarchy()
    for l in (2, 3):
        Cp = H["C"][l - 2]
        dev.replace_values(l, D.MG_OP_A, Cp.csr(np.full(Cp.nnz, np.nan + (1j * np.nan if vt != "float64" else 0)).astype(np.dtype(vt))))


def _refresh(dev, vt, a1, kind):
    from multigrid_jl_amd import device as D
    _poison(dev, vt)
    rc = _rap_status(dev, vt, a1, kind)
    D._check(dev.lib, rc, "mg_rap")
    return _state(dev, vt)


def _ref(T, level, R, A, P):
    key = (level, K.digest(R), K.digest(A), K.digest(P))
    if key not in _REFS:
        _REFS[key] = K.reference(T, R, A, P)
    return _REFS[key]


def _check(tag, vt, v, coarse, relax, kind, chunk, groups, exact):
    H = K.hierarchy()
    fine = [v["A"], coarse[0]]                      # level 2's operator is the device's own
    for l in (0, 1):
        T = H["T"][l]
        g = 1 if vt == "float64" else K.lane_groups(groups, chunk, H["C"][l].lens.max())
        share = K.check_entries(f"{tag} level {l + 1} -> {l + 2} ({g} groups)", vt, T, coarse[l],
                                _ref(T, l, v["R"][l], fine[l], v["P"][l]), groups=g, exact=exact)
        if not exact:
            SHARES[(vt, l + 1)] = max(SHARES.get((vt, l + 1), 0.0), share)
        K.check_relax(f"{tag} level {l + 1}", vt, kind, H["A"][l], fine[l], relax[l])
    return g


def _bits(state):
    return tuple(K.digest(a) for part in state for a in part)


def _run(mg, vt, chunk, groups, check=True):
    """One case on one resident handle; the bits of the crafted Jac refresh (for the comparisons between chunks)."""
    from multigrid_jl_amd import device as D
    key = (vt, chunk, groups)
    if key in _BITS and (not check or key in _CHECKED):      # (bits cached by an unchecked run do not stand in for the checks)
        return _BITS[key]
    p = _param(mg, vt)
    opts = {"rap_chunk": chunk}
    if groups:
        opts["rap_groups"] = groups
    dev = D.DeviceHierarchy(p, options=opts)
    p.device = dev
    try:
        assert isinstance(dev, {"float64": D.DeviceHierarchy, "complex128": D.ComplexDeviceHierarchy,
                                "complex64": D.ComplexSingleDeviceHierarchy}[vt])
        tag = f"{vt} chunk {chunk} groups {groups}"
        v = K.values(vt, "crafted")
        first = _refresh(dev, vt, v["A"], 0)
        if check:
            _check(tag + " Jac", vt, v, *first, 0, chunk, groups, False)
            spai = _refresh(dev, vt, v["A"], 1)
            _check(tag + " SPAI", vt, v, *spai, 1, chunk, groups, False)
            assert _bits(spai)[:2] == _bits(first)[:2]                       # (the operators do not depend on the vectors' kind)
            x = K.values(vt, "exact")
            for R, P, l in ((x["R"][0], x["P"][0], 1), (x["R"][1], x["P"][1], 2)):   # the exact family's P and R
                dev.replace_values(l, D.MG_OP_P, K.hierarchy()["P"][l - 1].csr(P))
                dev.replace_values(l, D.MG_OP_R, K.hierarchy()["R"][l - 1].csr(R))
            _check(tag + " exact", vt, x, *_refresh(dev, vt, x["A"], 0), 0, chunk, groups, True)
            for l in (1, 2):
                dev.replace_values(l, D.MG_OP_P, K.hierarchy()["P"][l - 1].csr(v["P"][l - 1]))
                dev.replace_values(l, D.MG_OP_R, K.hierarchy()["R"][l - 1].csr(v["R"][l - 1]))
            again = _refresh(dev, vt, v["A"], 0)                             # repeated: the same bits
            assert _bits(again) == _bits(first), tag
            print(f"\n{tag}: largest share of a bound so far " + ", ".join(f"{k[0]} level {k[1]}: {s:.3f}" for k, s in sorted(SHARES.items())))
    finally:
        mg.clear_(p)
    assert _BITS.get(key, _bits(first)) == _bits(first), tag      # (another handle of the same options: the same bits)
    _BITS[key] = _bits(first)
    if check:
        _CHECKED.add(key)
    return _BITS[key]


@pytest.mark.parametrize("vt,chunk,groups", CASES)
def test_crafted_products_entry_by_entry(mg, built, vt, chunk, groups):
    bits = _run(mg, vt, chunk, groups)
    if chunk == 5000:                                   # 5000 behaves as 2048
        assert bits == _run(mg, vt, 2048, groups, check=False)
    if vt == "float64" and chunk != 2048:               # float64: the order of an entry's sum does not depend on the chunk
        assert bits == _run(mg, vt, 2048, groups, check=False)


@pytest.mark.parametrize("vt", K.VTYPES)
def test_an_unsorted_coarse_row_is_refused_before_anything_is_written(mg, built, vt):
    """Two columns of one row of the middle operator swapped: MG_ERR_UNSUPPORTED, values and relaxation vectors untouched."""
    from multigrid_jl_amd import device as D
    p = _param(mg, vt)
    row = K.hierarchy()["marks"]["len2049"]
    M = p.As[1]
    s = M.indptr[row]
    M.indices[[s + 5, s + 900]] = M.indices[[s + 900, s + 5]]
    dev = D.DeviceHierarchy(p)
    p.device = dev
    try:
        before = _state(dev, vt)
        fine = np.asarray(dev.get_values(1, D.MG_OP_A)).copy()
        for kind in (0, 1):
            assert _rap_status(dev, vt, K.values(vt, "exact")["A"], kind) == MG_ERR_UNSUPPORTED
            assert b"do not ascend" in dev.lib.mg_last_error()
            assert _bits(_state(dev, vt)) == _bits(before)
            assert np.asarray(dev.get_values(1, D.MG_OP_A)).tobytes() == fine.tobytes()
        with pytest.raises(D.MGDeviceError):
            dev.replace_matrix(p, p.As[0])
    finally:
        mg.clear_(p)


def test_replace_matrix_in_hierarchy_takes_the_host_path_on_an_unsorted_coarse_row(mg, built):
    """A Poisson hierarchy whose middle operator has two stored columns of one row swapped (the same matrix): the device re-setup
    refuses, replaceMatrixInHierarchy computes on the host (its product has sorted rows again) and drops the handle, and the next
    solve uploads and matches the oracle."""
    from oracle import mg_oracle as orc
    A, mesh = mg.poisson_shifted([12, 12, 12])
    p = mg.getMGparam(np.float64, np.int64, 3, 8, 4, 1e-10, "Jac", 0.8, 2, 1, "V", "NoMUMPS", 0.5, 0.0)
    mg.MGsetup(A, mesh, p)
    M = p.As[1]
    s = M.indptr[40]
    for a in (M.indices, M.data):
        a[[s + 1, s + 4]] = a[[s + 4, s + 1]]
    b = mg.seeded_rhs(A)
    mg.to_device(p)                                      # (uploaded, no cycle: no kernel of the cycle reads the unsorted row)
    assert p.device is not None
    A2 = (A * 1.75).tocsr()
    mg.replaceMatrixInHierarchy(p, A2)
    assert p.device is None                              # the host path ran and released the handle
    want = (p.Rs[0] @ A2 @ p.Ps[0]).tocsr()
    assert abs(p.As[1] - want).max() <= 1e-13 * abs(want).max()
    x, xo, hist = np.zeros_like(b), np.zeros_like(b), {}
    mg.solveMG(p, b, x)
    orc.solveMG(p, b, xo, False, hist)
    assert np.abs(p.resvec - hist["resvec"]).max() <= 1e-10 * hist["resvec"][0] and np.abs(x - xo).max() <= 1e-10 * np.abs(xo).max()
    mg.clear_(p)


def test_operators_with_64_bit_row_pointers_are_refused(mg, built):
    from multigrid_jl_amd import device as D
    p = _param(mg, "float64")
    dev = D.DeviceHierarchy(p, options={"force_rowptr64": 1})
    p.device = dev
    try:
        assert _rap_status(dev, "float64", K.values("float64", "crafted")["A"], 0) == MG_ERR_UNSUPPORTED
        assert b"64-bit row pointers" in dev.lib.mg_last_error()
    finally:
        mg.clear_(p)
