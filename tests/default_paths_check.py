"""Row-by-row checks of device products against a long-double CSR reference (tests/test_default_paths.py).

Every product is checked componentwise: with k the length of a row and gamma_m = m u / (1 - m u), u = 2^-53,
    residual  r = b - A x              |got - ref| <= gamma_{k+1} (|b| + |A||x|)
    sweep     t = x + d.*(b - A x)     |got - ref| <= gamma_{k+3} (|x| + |d| (|b| + |A||x|))
    SpMV      y = alpha A x + beta y0  |got - ref| <= gamma_{k+2} (|beta||y0| + |alpha||A||x|)
A wrong value in a row of small magnitude fails here where a bound on the whole vector lets it pass.  The reference is a
CSR product in np.longdouble (64-bit significand: its own error is ~2^-11 of these bounds), chunked by rows over a few threads.

Device buffers are views into larger tensors with guard zones on both sides: output guards hold a sentinel bit pattern that
must survive bit for bit, input guards hold NaN (a read past either end poisons a row), and every output starts as NaN (an
unwritten row fails)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the reference needs an 80-bit (or wider) long double"
U = 2.0 ** -53
GUARD = 64                               # doubles on each side of a view (512 bytes: the view stays 16-byte aligned)
SENTINEL = np.int64(0x7FF4DEADBEEF5A5A)  # a signalling-NaN bit pattern: no kernel writes it
CHUNK = 1 << 14                          # rows per piece of the reference (its temporaries stay in cache)


def gamma(m):
    m = np.asarray(m, dtype=np.float64)
    return m * U / (1.0 - m * U)


def _threads():
    n = int(os.environ.get("OMP_NUM_THREADS") or 0) or len(os.sched_getaffinity(0))
    return max(1, min(16, n))


def _chunked(n, fn, chunk=None, work=None):
    """fn(r0, r1) over pieces of at most `chunk` rows (default CHUNK: cache-sized), in contiguous blocks, one per thread (numpy
    releases the GIL in these loops); the results in row order.  work: what decides whether threads pay (default: the rows)."""
    chunk = CHUNK if chunk is None else max(1, int(chunk))
    nt = _threads() if (n if work is None else work) > 4 * CHUNK else 1
    nt = max(1, min(nt, -(-n // chunk)))
    step = -(-n // nt)

    def block(b0):
        return [fn(r0, min(n, b0 + step, r0 + chunk)) for r0 in range(b0, min(n, b0 + step), chunk)]

    if nt == 1:
        return block(0)
    with ThreadPoolExecutor(nt) as ex:
        return [r for rs in ex.map(block, range(0, n, step)) for r in rs]


class Product:
    """A x in long double and |A||x| in double, row by row, for a CSR matrix A (empty rows give 0)."""

    def __init__(self, A, x):
        x = np.asarray(x, dtype=np.float64)
        n = A.shape[0]
        self.ax = np.empty(n, dtype=LD)
        self.abs = np.empty(n, dtype=np.float64)
        self.len = np.diff(A.indptr).astype(np.int64)
        ip, ci, va = A.indptr, A.indices, A.data

        def piece(r0, r1):
            s, e = int(ip[r0]), int(ip[r1])
            starts = ip[r0:r1] - s
            xs = x[ci[s:e]]
            prod = np.multiply(va[s:e], xs, dtype=LD)
            aprod = np.abs(va[s:e] * xs)
            if s == e:
                self.ax[r0:r1], self.abs[r0:r1] = 0, 0
                return
            nz = self.len[r0:r1] > 0
            if nz.all():
                self.ax[r0:r1] = np.add.reduceat(prod, starts)
                self.abs[r0:r1] = np.add.reduceat(aprod, starts)
            else:     # (reduceat over the starts of the non-empty rows: an empty row in between adds nothing)
                self.ax[r0:r1], self.abs[r0:r1] = 0, 0
                self.ax[r0:r1][nz] = np.add.reduceat(prod, starts[nz])
                self.abs[r0:r1][nz] = np.add.reduceat(aprod, starts[nz])

        # pieces of about 8 CHUNK entries (rows are never split: a row's sum does not depend on the pieces), threads by entries - an
        # SA-AMG level of 40 000 rows holds 10^8 of them
        _chunked(n, piece, chunk=CHUNK if A.nnz <= 8 * n else max(16, 8 * CHUNK * n // A.nnz), work=max(n, A.nnz // 8))


def _check(name, got, ref_bound):
    """ref_bound(r0, r1) -> (ref in long double, bound); every row must satisfy |got - ref| <= bound (NaN fails)."""
    got = np.asarray(got, dtype=np.float64)

    def piece(r0, r1):
        ref, bound = ref_bound(r0, r1)
        err = np.abs(got[r0:r1].astype(LD) - ref)
        bad = ~(err <= bound)
        if not bad.any():
            return None
        i = int(np.flatnonzero(bad)[0])
        return int(bad.sum()), r0 + i, float(got[r0 + i]), float(ref[i]), float(bound[i])

    fails = [f for f in _chunked(got.shape[0], piece) if f is not None]
    if fails:
        nbad = sum(f[0] for f in fails)
        _, row, g, r, bd = fails[0]
        raise AssertionError(f"{name}: {nbad} of {got.shape[0]} rows outside the componentwise bound; first row {row}: "
                             f"got {g!r}, reference {r!r}, bound {bd!r}")
    return got.shape[0]


def check_residual(name, got, b, prod):
    """got = b - A x, prod = Product(A, x)."""
    b = np.asarray(b, dtype=np.float64)
    return _check(name, got, lambda r0, r1: (b[r0:r1].astype(LD) - prod.ax[r0:r1],
                                             gamma(prod.len[r0:r1] + 1) * (np.abs(b[r0:r1]) + prod.abs[r0:r1])))


def check_sweep(name, got, x, d, b, prod):
    """got = x + d.*(b - A x), prod = Product(A, x)."""
    x, d, b = (np.asarray(v, dtype=np.float64) for v in (x, d, b))
    return _check(name, got, lambda r0, r1: (
        x[r0:r1].astype(LD) + d[r0:r1].astype(LD) * (b[r0:r1].astype(LD) - prod.ax[r0:r1]),
        gamma(prod.len[r0:r1] + 3) * (np.abs(x[r0:r1]) + np.abs(d[r0:r1]) * (np.abs(b[r0:r1]) + prod.abs[r0:r1]))))


def check_spmv(name, got, alpha, prod, beta=0.0, y0=None):
    """got = alpha A x + beta y0, prod = Product(A, x); beta = 0 does not read y0 (it may be NaN)."""
    y0 = None if beta == 0.0 else np.asarray(y0, dtype=np.float64)

    def ref_bound(r0, r1):
        ref = LD(alpha) * prod.ax[r0:r1]
        scale = abs(alpha) * prod.abs[r0:r1]
        if y0 is not None:
            ref = ref + LD(beta) * y0[r0:r1].astype(LD)
            scale = scale + abs(beta) * np.abs(y0[r0:r1])
        return ref, gamma(prod.len[r0:r1] + 2) * scale

    return _check(name, got, ref_bound)


def check_xpdr(name, got, t, d, r):
    """got = t + d.*r from the device's own t and r."""
    t, d, r = (np.asarray(v, dtype=np.float64) for v in (t, d, r))
    return _check(name, got, lambda r0, r1: (t[r0:r1].astype(LD) + d[r0:r1].astype(LD) * r[r0:r1].astype(LD),
                                             gamma(2) * (np.abs(t[r0:r1]) + np.abs(d[r0:r1] * r[r0:r1]))))


def check_block(name, kind, got, A, X, cols=None, B=None, d=None, alpha=1.0, beta=0.0, Y0=None, prods=None):
    """A block of right-hand sides, column by column: got, X, B, Y0 are (rows, nrhs) arrays (any strides), kind is
    "residual" (B - A X), "sweep" (X + d.*(B - A X)) or "spmv" (alpha A X + beta Y0).  Every column of `cols` (default: all)
    is checked against Product(A, X[:, j]) with the single-vector bounds.  A column of X that is exactly zero must give
    exactly B (residual) or exactly beta * Y0 (spmv; 0 for beta = 0, where Y0 may be NaN): compared by value, so a NaN fails and
    -0.0 equals 0.0.  prods: a dict that keeps the Product of a column from one call to the next (same A and X)."""
    got, X = np.asarray(got, dtype=np.float64), np.asarray(X, dtype=np.float64)
    assert got.ndim == 2 and X.ndim == 2 and got.shape == (A.shape[0], X.shape[1]) and X.shape[0] == A.shape[1], (got.shape, X.shape, A.shape)
    rows = 0
    for j in (range(X.shape[1]) if cols is None else cols):
        x, g = np.ascontiguousarray(X[:, j]), np.ascontiguousarray(got[:, j])
        col = lambda M: None if M is None else np.ascontiguousarray(M[:, j])
        if kind != "sweep" and not x.any():
            want = col(B) if kind == "residual" else (np.zeros_like(g) if beta == 0.0 else beta * col(Y0))
            same = g == want
            if not same.all():
                i = int(np.flatnonzero(~same)[0])
                raise AssertionError(f"{name} column {j} (x = 0): row {i} is {g[i]!r}, not exactly {want[i]!r}")
            rows += g.shape[0]
            continue
        pr = prods.get(j) if prods is not None else None
        if pr is None:
            pr = Product(A, x)
            if prods is not None:
                prods[j] = pr
        if kind == "residual":
            rows += check_residual(f"{name} column {j}", g, col(B), pr)
        elif kind == "sweep":
            rows += check_sweep(f"{name} column {j}", g, x, d, col(B), pr)
        else:
            assert kind == "spmv", kind
            rows += check_spmv(f"{name} column {j}", g, alpha, pr, beta, col(Y0))
    return rows


def norm_ld(v):
    """sqrt(sum v^2) in long double."""
    v = np.asarray(v, dtype=np.float64)
    parts = _chunked(v.shape[0], lambda r0, r1: np.sum(np.square(v[r0:r1].astype(LD))))
    return float(np.sqrt(np.sum(np.array(parts, dtype=LD))))


# ---- guarded device buffers ------------------------------------------------------------------------------------------
class Guarded:
    """A length-n float64 view into a CUDA tensor of n + 2 GUARD doubles.  out=True: guards hold SENTINEL and the view NaN;
    out=False: guards hold NaN and the view `data`."""

    def __init__(self, n, data=None, out=True):
        import torch
        self.n = int(n)
        self.base = torch.empty(self.n + 2 * GUARD, dtype=torch.float64, device="cuda")
        self.out = out
        if out:
            self.base.view(torch.int64).fill_(int(SENTINEL))
            self.v = self.base[GUARD:GUARD + self.n]
            self.v.fill_(float("nan"))
        else:
            self.base.fill_(float("nan"))
            self.v = self.base[GUARD:GUARD + self.n]
            self.v.copy_(torch.from_numpy(np.ascontiguousarray(data, dtype=np.float64)))
        assert self.v.data_ptr() % 16 == 0

    @classmethod
    def block(cls, n, nrhs, data=None, out=True):
        """A block of nrhs columns as the device-resident entry points take it: one buffer of n * nrhs doubles between the
        guard zones, entry (i, j) at i * nrhs + j (the host-pointer entry points transpose a column-major n x nrhs host block
        into this).  data: an (n, nrhs) array.  host2d() returns the checked view as an (n, nrhs) array."""
        if data is not None:
            data = np.ascontiguousarray(np.asarray(data, dtype=np.float64).reshape(int(n), int(nrhs)))   # C order: i * nrhs + j
        g = cls(int(n) * int(nrhs), None if data is None else data.ravel(), out)
        g.shape = (int(n), int(nrhs))
        return g

    def host2d(self):
        return self.host().reshape(self.shape)

    def host_guards(self):
        """Check the guard zones alone (no copy of the view)."""
        host_checked(np.concatenate([self.base[:GUARD].cpu().numpy(), self.base[self.base.shape[0] - GUARD:].cpu().numpy()]), self.out)

    def host(self):
        """The view on the host, after checking both guard zones bit for bit (outputs) or that they are still NaN (inputs)."""
        return host_checked(self.base.cpu().numpy(), self.out)


def host_checked(base, out=True):
    """The view part of a host copy of a guarded buffer; raises if a guard word changed."""
    lo, hi = base[:GUARD], base[base.shape[0] - GUARD:]
    if out:
        ok = np.all(lo.view(np.int64) == SENTINEL) and np.all(hi.view(np.int64) == SENTINEL)
    else:
        ok = np.all(np.isnan(lo)) and np.all(np.isnan(hi))
    if not ok:
        raise AssertionError("a guard word next to a device buffer changed: a write outside the buffer")
    return base[GUARD:base.shape[0] - GUARD]
