"""Shared inputs and the comparand of the Schwarz tests (test infrastructure): an independent numpy statement of the
reference's cellColor (Vanka.jl:105-130), setupDDSerial (DDSerial.jl:81-106) and solveDDSerial (DDSerial.jl:108-139) with
scipy's splu as the sub-domain solver.  It shares no code with multigrid.jl_amd/domain_decomposition.py; the index
lists come from dd_indices (tested on their own).  Used by tests/test_dd_host.py and tests/test_dd_gpu.py."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def cell_color(i):
    """Vanka.jl:105-130 as arithmetic: the last index is the fastest bit, odd indices come first."""
    c = 0
    for k in i:
        c = 2 * c + (1 - int(k) % 2)
    return c + 1


class Restated:
    """Index lists, colours and factored sub-domain matrices A[IIp, IIp]."""

    def __init__(self, mg, A, n, numDomains, overlap):
        self.A = sp.csr_matrix(A)
        self.numDomains = [int(k) for k in numDomains]
        self.dim = len(self.numDomains)
        self.lists, self.colors, self.lus = [], [], []
        for ii in range(1, int(np.prod(numDomains)) + 1):
            loc = mg.cs2loc(ii, numDomains)
            I = np.asarray(mg.getNodalIndicesOfCell(numDomains, overlap, loc, np.asarray(n)), dtype=np.int64) - 1
            self.lists.append(I)
            self.colors.append(cell_color(loc))
            self.lus.append(spla.splu(sp.csc_matrix(self.A[I][:, I])))

    def sweep(self, b, x, niter=1, doTranspose=0):
        """solveDDSerial: x in place; the residual always uses A, doTranspose reaches the sub-solves (the adjoint)."""
        for _ in range(niter):
            for color in range(1, 2 ** self.dim + 1):
                for I, c, lu in zip(self.lists, self.colors, self.lus):
                    if c != color:
                        continue
                    r = b[I] - self.A[I] @ x
                    x[I] += lu.solve(r, "H") if doTranspose else lu.solve(r)
        return x

    def independent(self):
        """colour -> are its members independent, by brute force on sets: lists pairwise disjoint, and the columns stored
        in one member's rows disjoint from every other member's list."""
        out = {}
        for color in sorted(set(self.colors)):
            mem = [k for k, c in enumerate(self.colors) if c == color]
            sets = [set(self.lists[k].tolist()) for k in mem]
            reads = [set(self.A[self.lists[k]].indices.tolist()) for k in mem]
            out[color] = all(not (sets[a] & sets[b]) and not (reads[a] & sets[b])
                             for a in range(len(mem)) for b in range(len(mem)) if a != b)
        return out


def poisson(mg, n, seed=1):
    """testDDPoisson.jl:22-40: A = G'G + 1e-5 * opnorm(A, 1) * I on the nodal grid of n cells, b = randn (seeded here)."""
    mesh = mg.getRegularMesh([0.0, 1.0] * len(n), list(n))
    G = mg.getNodalGradientMatrix(mesh)
    A = (G.T @ G).tocsr()
    A = (A + 1e-5 * abs(A).sum(axis=0).max() * sp.identity(A.shape[0], format="csr")).tocsr()
    A.sort_indices()
    b = np.random.default_rng(seed).standard_normal(A.shape[0])
    return A, mesh, b


def dd_param(mg, A, mesh, numDomains, overlap, VAL=np.float64):
    """The product's DDparam on the same problem, set up."""
    Ainv = mg.ParallelJuliaSolver.getParallelJuliaSolver(VAL, np.int64, numCores=2, backend=1)
    p = mg.getDomainDecompositionParam(VAL, np.int64, mesh, numDomains, overlap, mg.getNodalIndicesOfCell, Ainv)
    return mg.setupDDSerial(A, p)


@functools.lru_cache(maxsize=None)
def reference_case(mg):
    """The reference's own problem (32^2, boxes [8,8], overlap [1,1]) with its restatement: (A, mesh, b, Restated)."""
    A, mesh, b = poisson(mg, [32, 32])
    return A, mesh, b, Restated(mg, A, [32, 32], [8, 8], [1, 1])


def gmres_count(A, b, M, rtol=1e-10):
    """scipy gmres with the preconditioner r -> M(r): (x, inner iterations)."""
    its = []
    op = spla.LinearOperator(A.shape, matvec=M, dtype=A.dtype)
    x, info = spla.gmres(A, b, M=op, rtol=rtol, atol=0.0, restart=60, maxiter=10, callback=lambda r: its.append(r),
                         callback_type="pr_norm")
    assert info == 0
    return x, len(its)
