"""-m gpu: the complex cycle's own kernels - SMOOTH, RESID with and without the sumsq partial, cx_dscale / cx_dscale_blk - on the
awkward row blocks of tests/complex_awkward_cases.py: empty rows, full 1024-entry chunks, blocks of MAXROWS rows (one without any
entry) and the one-long-row branch of cx_csr_stream_spmv and cx_csr_stream_spmm, in ComplexF64 and ComplexF32, on 32- and 64-bit row
pointers, for one vector and for blocks of every lane-group width.

  * hierarchy ``sweeps`` (P holds stored zeros): a cycle is a chain of sweeps, checked row by row against the long-double chain under
    the derived sweep bound; repeated runs give the same bits; block buffers sit between guard zones;
  * hierarchy ``full``: two cycles against the complex oracles at the project's own tolerances (1e-12 in the max norm per vector or
    column; the ComplexF32 rule of tests/test_complex_single_gpu.py), with the dense-inverse and the sparse-factor coarsest solve;
  * solveMG's resvec (the per-row-block sumsq partials, long-row blocks included) against the long-double norms under the derived
    norm bound.
Every test prints the device's worst ratio of error to bound."""
import numpy as np
import pytest
import torch

import complex_awkward_cases as ac
import complex_block_oracle as cb
import complex_oracle as corc
import complex_single_oracle as cs

pytestmark = pytest.mark.gpu

N = ac.N
GUARD = 64                               # complex values on each side of a block (1 KiB: the view stays 16-byte aligned)
SENTINEL = 0x7FF4DEADBEEF5A5A            # a signalling-NaN bit pattern: no kernel writes it (tests/default_paths_check.py)
BLOCK_SWEEPS = (2, 2)
FULL_SWEEPS = (2, 1)


@pytest.fixture(scope="module")
def devs(mg, built):
    """(hierarchy, param, device hierarchy) per (kind, precision, row-pointer width, coarsest form), made on first use and shared."""
    made = {}

    def get(kind, single, wide, sparse=False):
        key = (kind, bool(single), int(wide), bool(sparse))
        if key not in made:
            h = ac.hierarchy(kind, single)
            p = h.param(mg, *FULL_SWEEPS)
            dev = mg.device.DeviceHierarchy(p, options={"force_rowptr64": wide})
            made[key] = (h, p, dev)
            if sparse:                               # the coarsest solve from the complex sparse factors
                dev._set_coarse(p, force_sparse=True)
                assert dev.lib.mg_finalize(dev.handle) == 0
            assert dev.coarse_form()["kind"] == (1 if sparse else 0)
        return made[key]

    yield get
    for _, _, d in made.values():
        d.close()


def _sweeps(dev, p, pre, post):
    ac.set_sweeps(p, pre, post)
    dev.sync_schedule(p)


_refs = {}


def _shared(key, make):
    """A reference computed once and shared among the cases that need it (nothing modifies it)."""
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


def _chain(h, tag, b, x0, pre, post, from_zero):
    return _shared(("chain", h.single, tag, pre, post, from_zero),
                   lambda: (ac.sweep_chain(h, b, x0, pre, post, from_zero), ac.sweep_bound(h, b, x0, pre, post, from_zero)))


# ---- guarded device blocks -----------------------------------------------------------------------------------------------------------
class GuardedBlock:
    """A contiguous [n, k] complex128 view inside a larger device tensor.  out=True: the guards hold SENTINEL and the view NaN
    (or `data`); out=False: the guards hold NaN and the view `data`."""

    def __init__(self, n, k, data=None, out=True):
        self.out = out
        self.base = torch.empty(n * k + 2 * GUARD, dtype=torch.complex128, device="cuda")
        real = torch.view_as_real(self.base)
        if out:
            real.view(torch.int64).fill_(SENTINEL)
        else:
            real.fill_(float("nan"))
        self.v = self.base[GUARD:GUARD + n * k].view(n, k)
        if data is None:
            torch.view_as_real(self.v).fill_(float("nan"))
        else:
            self.v.copy_(torch.from_numpy(np.ascontiguousarray(data, dtype=np.complex128)))
        assert self.v.is_contiguous() and self.v.data_ptr() % 16 == 0 and self.v.data_ptr() != self.base.data_ptr()

    def host(self):
        """The view on the host, after checking both guard zones bit for bit (outputs) or that they are still NaN (inputs)."""
        torch.cuda.synchronize()
        base = self.base.cpu().numpy()
        lo, hi = base[:GUARD], base[base.shape[0] - GUARD:]
        if self.out:
            ok = np.all(lo.view(np.int64) == SENTINEL) and np.all(hi.view(np.int64) == SENTINEL)
        else:
            ok = np.all(np.isnan(lo.view(np.float64))) and np.all(np.isnan(hi.view(np.float64)))
        assert ok, "a guard word next to a device block changed: a write outside the block"
        return base[GUARD:base.shape[0] - GUARD].reshape(tuple(self.v.shape)).copy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


# ---- 1. sweeps row by row, one vector ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("from_zero", [True, False])
@pytest.mark.parametrize("pre,post", [(1, 1), (2, 2)])
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("single", [False, True])
def test_sweeps_row_by_row_vector(devs, single, wide, pre, post, from_zero):
    h, p, dev = devs("sweeps", single, wide)
    _sweeps(dev, p, pre, post)
    b, x0 = ac.vector(1, single), ac.vector(2, single)
    ref, E = _chain(h, "v", b, x0, pre, post, from_zero)

    def run():
        x = np.full(N, np.nan + 1j * np.nan, dtype=h.cdtype) if from_zero else x0.copy()      # from zero: x is not read
        assert dev.cycle(b, x, 1 if from_zero else 0) is x
        return x

    x = run()
    worst = ac.check_rows(f"sweeps vector single={single} wide={wide} ({pre},{post}) from_zero={from_zero}", x, ref, E)
    print(f"  vector {'CF32' if single else 'CF64'} rowptr64={wide} ({pre},{post}) from_zero={from_zero}: worst row {worst:.3f} of its bound")
    assert np.array_equal(run(), x)                                     # a second run: the same bits


# ---- 2. sweeps row by row, blocks ----------------------------------------------------------------------------------------------------
def _block_case(h, k, from_zero):
    B = ac.block(1, h.single, k)
    X0 = ac.block(2, h.single, k)
    ref, E = _chain(h, ("b", k), B, X0, *BLOCK_SWEEPS, from_zero)
    return B, X0, ref, E


def _run_block_sweeps(h, p, dev, k, from_zero, tag):
    _sweeps(dev, p, *BLOCK_SWEEPS)
    B, X0, ref, E = _block_case(h, k, from_zero)
    Bg = GuardedBlock(N, k, B, out=False)
    Xg = GuardedBlock(N, k, None if from_zero else X0, out=True)
    dev.block_cycle_dev(Bg.v, Xg.v, 1 if from_zero else 0)
    X = Xg.host()
    assert _same_bits(Bg.host(), B)                                     # B unchanged bit for bit, its NaN guards still NaN
    worst = ac.check_rows(tag, X, ref, E)
    zc = ac.zero_column(k)
    if zc is not None:
        assert not E[:, zc].any() and not X[:, zc].any()                # the all-zero column: exact zeros
    print(f"  {tag}: worst row {worst:.3f} of its bound")
    X2 = GuardedBlock(N, k, None if from_zero else X0, out=True)
    dev.block_cycle_dev(Bg.v, X2.v, 1 if from_zero else 0)
    assert _same_bits(X2.host(), X)                                     # a second run: the same bits


@pytest.mark.parametrize("from_zero", [True, False])
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("k", ac.KS)
def test_sweeps_row_by_row_blocks(devs, k, wide, from_zero):
    h, p, dev = devs("sweeps", False, wide)
    _run_block_sweeps(h, p, dev, k, from_zero, f"blocks CF64 k={k} rowptr64={wide} from_zero={from_zero}")


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("k", ac.KS)
def test_sweeps_row_by_row_blocks_single(devs, k, wide):
    """block_cycle_dev on a CF32 hierarchy: the mixed closure from zero on a complex128 block that single represents exactly; the
    result is the single chain widened."""
    h, p, dev = devs("sweeps", True, wide)
    _run_block_sweeps(h, p, dev, k, True, f"blocks CF32 k={k} rowptr64={wide} from_zero=True")


# ---- 3. full cycles against the oracles ----------------------------------------------------------------------------------------------
def _columns_close(X, Xo, tol):
    """tests/test_complex_block_gpu.py's rule; returns the worst column's relative distance."""
    worst = 0.0
    for j in range(X.shape[1]):
        scale = np.abs(Xo[:, j]).max()
        if scale == 0.0:
            assert not X[:, j].any(), j                                 # a zero column stays exactly zero
        else:
            e = np.abs(X[:, j] - Xo[:, j]).max() / scale
            assert e <= tol, (j, e)
            worst = max(worst, e)
    return worst


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("wide", [0, 1])
def test_full_cycle_vector_against_complex_oracle(devs, wide, sparse):
    h, p, dev = devs("full", False, wide, sparse)
    _sweeps(dev, p, *FULL_SWEEPS)
    b = ac.vector(3, False)

    def oracle():
        x1 = corc.recursiveCycle(p, b, np.zeros_like(b), 1).copy()
        return x1, corc.recursiveCycle(p, b, x1.copy(), 1).copy()

    xo1, xo2 = _shared(("full-vector",), oracle)
    x = np.zeros_like(b)
    dev.cycle(b, x, 1)
    e1 = np.abs(x - xo1).max() / np.abs(xo1).max()
    dev.cycle(b, x, -1)
    e2 = np.abs(x - xo2).max() / np.abs(xo2).max()
    print(f"  full CF64 vector rowptr64={wide} sparse={sparse}: {e1:.2e} from zero, {e2:.2e} from the iterate (allowed 1e-12)")
    assert e1 <= 1e-12 and e2 <= 1e-12


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("k", ac.KS)
def test_full_cycle_blocks_against_block_oracle(devs, k, wide, sparse):
    h, p, dev = devs("full", False, wide, sparse)
    _sweeps(dev, p, *FULL_SWEEPS)
    B = np.asfortranarray(ac.block(3, False, k))

    def oracle():
        X1 = cb.block_cycle(p, B, np.zeros((N, k), dtype=np.complex128)).copy()
        return X1, cb.block_cycle(p, B, X1.copy()).copy()

    Xo1, Xo2 = _shared(("full-block", k), oracle)
    X = np.zeros((N, k), dtype=np.complex128, order="F")
    assert dev.block_cycle(B, X, 1) is X
    e1 = _columns_close(X, Xo1, 1e-12)
    Xfirst = X.copy(order="F")
    dev.block_cycle(B, X, -1)                                           # x != 0: decided for the whole block
    e2 = _columns_close(X, Xo2, 1e-12)
    print(f"  full CF64 blocks k={k} rowptr64={wide} sparse={sparse}: worst column {e1:.2e} from zero, {e2:.2e} from the iterate (allowed 1e-12)")
    # the device form on row-major blocks: the same bits, from zero and from the iterate
    Bg = GuardedBlock(N, k, B, out=False)
    Xg = GuardedBlock(N, k, None, out=True)
    dev.block_cycle_dev(Bg.v, Xg.v, 1)
    assert _same_bits(Xg.host(), np.ascontiguousarray(Xfirst))
    dev.block_cycle_dev(Bg.v, Xg.v, 0)
    assert _same_bits(Xg.host(), np.ascontiguousarray(X)) and _same_bits(Bg.host(), np.ascontiguousarray(B))


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("wide", [0, 1])
def test_full_cycle_vector_single_against_the_rounded_double_cycle(devs, wide, sparse):
    """tests/test_complex_single_gpu.py's rule: e_ref < 64 U32 and e_dev <= 4 e_ref against the double cycle on the rounded hierarchy."""
    h, p, dev = devs("full", True, wide, sparse)
    _sweeps(dev, p, *FULL_SWEEPS)
    b = ac.vector(3, True)

    def oracle():
        pr = cs.rounded(p)
        xs1 = cs.recursiveCycle(p, b, np.zeros_like(b), 1).copy()
        xs2 = cs.recursiveCycle(p, b, xs1.copy(), 1).copy()
        xo1 = corc.recursiveCycle(pr, b.astype(np.complex128), np.zeros(N, dtype=np.complex128), 1).copy()
        xo2 = corc.recursiveCycle(pr, b.astype(np.complex128), xo1.copy(), 1).copy()
        return (xs1, xo1), (xs2, xo2)

    x = np.zeros_like(b)
    for i, (xz, (xs, xo)) in enumerate(zip((1, -1), _shared(("full-vector-single",), oracle))):
        dev.cycle(b, x, xz)
        e_ref, e_dev = cs.rel2(xs, xo), cs.rel2(x, xo)
        print(f"  full CF32 vector rowptr64={wide} sparse={sparse} cycle {i + 1}: restatement {e_ref:.3e}, device {e_dev:.3e} from the double cycle")
        assert e_ref < 64 * ac.U32
        assert e_dev <= 4 * e_ref


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("k", ac.KS)
def test_full_cycle_blocks_single_against_the_restatement(devs, k, wide, sparse):
    h, p, dev = devs("full", True, wide, sparse)
    _sweeps(dev, p, *FULL_SWEEPS)
    B = ac.block(3, True, k)

    def oracle():
        M = cs.preconditioner(p)
        return [M(B[:, j]).copy() for j in range(k)]

    Zo = _shared(("full-block-single", k), oracle)
    Bg = GuardedBlock(N, k, B, out=False)
    Xg = GuardedBlock(N, k, None, out=True)
    dev.block_cycle_dev(Bg.v, Xg.v, 1)
    X = Xg.host()
    assert _same_bits(Bg.host(), B)
    worst = 0.0
    for j in range(k):
        if not Zo[j].any():
            assert j == ac.zero_column(k) and not X[:, j].any()         # the all-zero column: exact zeros
            continue
        e = cs.rel2(X[:, j], Zo[j])
        assert e < 64 * ac.U32, (j, e)
        worst = max(worst, e)
    print(f"  full CF32 blocks k={k} rowptr64={wide} sparse={sparse}: worst column {worst:.3e} from the restatement (allowed {64 * ac.U32:.3e})")


# ---- 4. the norm partials ------------------------------------------------------------------------------------------------------------
def _check_norm(tag, got, ref_bound):
    ref, bound = ref_bound
    ratio = abs(got - ref) / bound
    print(f"  {tag}: {got!r} against {ref!r}, {ratio:.2e} of the bound ({bound / ref:.1e} relative)")
    assert ratio <= 1.0, (tag, got, ref, bound)                         # (NaN fails)


@pytest.mark.parametrize("from_zero", [True, False])
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("single", [False, True])
def test_resvec_vector_against_long_double_norms(devs, single, wide, from_zero):
    h, p, dev = devs("full", single, wide)
    _sweeps(dev, p, *FULL_SWEEPS)
    b, x0 = ac.vector(3, single), ac.vector(4, single)
    x = np.zeros_like(b) if from_zero else x0.copy()
    _, it, resvec = dev.solve(b, x, 0.0, 1)
    assert it == 1 and resvec.shape == (2,) and x.dtype == h.cdtype
    tag = f"resvec {'CF32' if single else 'CF64'} rowptr64={wide} from_zero={from_zero}"
    _check_norm(tag + " [0]", resvec[0], ac.residual_norm(h, b, None if from_zero else x0))
    _check_norm(tag + " [1]", resvec[1], ac.residual_norm(h, b, x))


@pytest.mark.parametrize("from_zero", [True, False])
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("k", [3, 16])
def test_resvec_blocks_against_long_double_norms(devs, k, wide, from_zero):
    h, p, dev = devs("full", False, wide)
    _sweeps(dev, p, *FULL_SWEEPS)
    B, X0 = np.asfortranarray(ac.block(3, False, k)), ac.block(4, False, k)
    X = np.zeros((N, k), dtype=np.complex128, order="F") if from_zero else np.asfortranarray(X0)
    _, it, resvec = dev.block_solve(B, X, 0.0, 1)
    assert it == 1 and resvec.shape == (2,)
    tag = f"resvec blocks k={k} rowptr64={wide} from_zero={from_zero}"
    _check_norm(tag + " [0]", resvec[0], ac.residual_norm(h, B, None if from_zero else X0))
    _check_norm(tag + " [1]", resvec[1], ac.residual_norm(h, B, X))
