"""Shared by the Vanka tests: a staggered mixed operator in the unknown ordering of Vanka.jl, a numpy restatement of the
Julia serial path of RelaxVankaFacesColor (Vanka.jl:383-425, line by line: the snapshot per colour, the per-call y of ADD),
a numpy V-cycle on general sparse As / Ps / Rs that calls it, and the seeded cases of the reference fixture."""
import os

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_binaries", "vanka_outputs.npz")

FULL_VANKA_RB, ECON_VANKA_RB, FULL_VANKA_LEX, FULL_VANKA_ADD = 1, 3, 4, 5
LAMBDA, MU = 1.0, 1.0      # C = -diag(1/(lambda+mu)), as in testGMGforElasticityVanka.jl


def _d1(n, h):
    """1-D node -> cell difference, n x (n+1)."""
    return sp.diags([-np.ones(n), np.ones(n)], [0, 1], shape=(n, n + 1), format="csr") / h


def _kron(ops):
    K = ops[0]
    for M in ops[1:]:
        K = sp.kron(M, K, format="csr")
    return sp.csr_matrix(K)


def _lap1(m, h, nodal):
    """1-D Laplacian of m points: nodal (Dirichlet-like, full stencil) or cell-centred (Neumann-like ends)."""
    if nodal:
        D = _d1(m - 1, h)
        return (D.T @ D + sp.diags([np.r_[1.0, np.zeros(m - 2), 1.0] / h ** 2], [0])).tocsr()
    if m == 1:
        return sp.csr_matrix([[2.0 / h ** 2]])
    D = sp.diags([-np.ones(m - 1), np.ones(m - 1)], [0, 1], shape=(m - 1, m), format="csr") / h
    return (D.T @ D + sp.diags([np.r_[2.0, np.zeros(m - 2), 2.0] / h ** 2], [0])).tocsr()


def mixed_operator(n, includePressure=True, omega=None, mass=1e-2, lam=LAMBDA, mu=MU):
    """H = [A D'; -D -C] (faces only: A) on a unit-spaced mesh of n cells: A = mu * face vector-Laplacian + mass,
    D = cell divergence, C = -diag(1/(lam+mu)).  omega: adds -omega^2 (1 - 0.1i) times the face mass (complex)."""
    n = [int(k) for k in n]
    dim = len(n)
    h = 1.0
    blocks, divs = [], []
    for j in range(dim):
        size = [n[k] + (1 if k == j else 0) for k in range(dim)]
        L = sp.csr_matrix((int(np.prod(size)),) * 2)
        for k in range(dim):
            ops = [sp.identity(size[q], format="csr") for q in range(dim)]
            ops[k] = _lap1(size[k], h, nodal=(k == j))
            L = L + _kron(ops)
        Aj = mu * L + mass * sp.identity(L.shape[0], format="csr")
        if omega is not None:
            Aj = Aj.astype(np.complex128) - (omega ** 2) * (1.0 - 0.1j) * sp.identity(L.shape[0], format="csr")
        blocks.append(Aj)
        ops = [sp.identity(n[q], format="csr") for q in range(dim)]
        ops[j] = _d1(n[j], h)
        divs.append(_kron(ops))
    A = sp.block_diag(blocks, format="csr")
    if not includePressure:
        H = A
    else:
        D = sp.hstack(divs, format="csr")
        cells = int(np.prod(n))
        C = -sp.identity(cells, format="csr") / (lam + mu)
        H = sp.bmat([[A, D.T], [-D, -C]], format="csr")
    H = sp.csr_matrix(H)
    H.sort_indices()
    return H


def seeded(n_unknowns, seed, cx=False):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n_unknowns)
    if cx:
        v = v + 1j * rng.standard_normal(n_unknowns)
    return v


_ROWS = {}


# ---- the restatement -----------------------------------------------------------------------------------------------
def cs2loc(ii, n):
    ii -= 1
    loc = []
    for d in range(len(n)):
        loc.append(ii % n[d] + 1)
        ii //= n[d]
    return loc


def cell_color(i):
    if len(i) == 2:
        if i[0] % 2 == 1:
            return 1 if i[1] % 2 == 1 else 2
        return 3 if i[1] % 2 == 1 else 4
    if i[0] % 2 == 1:
        if i[1] % 2 == 1:
            return 1 if i[2] % 2 == 1 else 2
        return 3 if i[2] % 2 == 1 else 4
    if i[1] % 2 == 1:
        return 5 if i[2] % 2 == 1 else 6
    return 7 if i[2] % 2 == 1 else 8


def block_size(n, ip):
    n = [int(k) for k in n]
    if len(n) == 2:
        return (5 if ip else 4), [(n[0] + 1) * n[1], n[0] * (n[1] + 1)]
    return (7 if ip else 6), [(n[0] + 1) * n[1] * n[2], n[0] * (n[1] + 1) * n[2], n[0] * n[1] * (n[2] + 1)]


def cell_unknowns(i, n, nf, ip):
    """getVankaVariablesOfCell (Vanka.jl:45-95), 1-based."""
    if len(i) == 2:
        t1 = i[0] + (i[1] - 1) * (n[0] + 1)
        t2 = nf[0] + i[0] + (i[1] - 1) * n[0]
        I = [t1, t1 + 1, t2, t2 + n[0]]
        if ip:
            I.append(nf[1] + t2)
        return I
    l3 = lambda nn: i[0] + (i[1] - 1) * nn[0] + (i[2] - 1) * nn[0] * nn[1]
    t1 = l3([n[0] + 1, n[1], n[2]])
    t2 = nf[0] + l3([n[0], n[1] + 1, n[2]])
    t3 = nf[0] + nf[1] + l3(n)
    I = [t1, t1 + 1, t2, t2 + n[0], t3, t3 + n[0] * n[1]]
    if ip:
        I.append(nf[2] + t3)
    return I


def all_unknowns(n, ip):
    n = [int(k) for k in n]
    bs, nf = block_size(n, ip)
    return np.array([cell_unknowns(cs2loc(ii, n), n, nf, ip) for ii in range(1, int(np.prod(n)) + 1)], dtype=np.int64)


def restate_relax(A, x, b, D, numit, n, ip, vtype):
    """The Julia serial path, in place on x; D is LocalBlocks (bs^2, cells).  r = b[I] - A[I, :] y, x[I] += reshape(D_i)' r with
    the single-precision block promoted to double."""
    n = [int(k) for k in n]
    bs, nf = block_size(n, ip)
    I_all = all_unknowns(n, ip) - 1
    cells = I_all.shape[0]
    Mall = np.conj(np.asarray(D).T.reshape(cells, bs, bs)).astype(x.dtype)   # reshape(D[:, i], bs, bs)' : [t, j] = conj(D[j + t bs])
    colours = np.array([cell_color(cs2loc(ii, n)) for ii in range(1, cells + 1)])
    key = (id(A), tuple(n), ip)
    if key not in _ROWS:                     # (the cells' row slices of an operator, cut once: the cycles reuse them)
        Ac = sp.csr_matrix(A)
        _ROWS[key] = (A, [Ac[I_all[c], :] for c in range(cells)])
    rows = _ROWS[key][1]
    if vtype == FULL_VANKA_ADD:
        y = x.copy()
        for _ in range(numit):
            for c in range(cells):
                I = I_all[c]
                r = b[I] - rows[c] @ y
                x[I] = x[I] + Mall[c] @ r
        return x
    assert vtype in (FULL_VANKA_RB, ECON_VANKA_RB)
    y = x.copy()
    for _ in range(numit):
        for color in range(1, 2 ** len(n) + 1):
            y[:] = x
            for c in np.nonzero(colours == color)[0]:
                I = I_all[c]
                r = b[I] - rows[c] @ y
                x[I] = x[I] + Mall[c] @ r
    return x


def restate_vcycle(As, Ps, Rs, Ds, meshes_n, ip, vtype, lu, b, x, x_zero, npre=1, npost=1, cycle="V", level=0):
    """recursiveCycle (MGcycle.jl) with Vanka relaxation on every non-coarsest level and a direct coarsest solve."""
    if level == len(As) - 1:
        return lu.solve(b)
    if x_zero:
        x = np.zeros_like(b)
    x = restate_relax(As[level], x.copy(), b, Ds[level], npre, meshes_n[level], ip, vtype)
    r = b - As[level] @ x
    bc = Rs[level] @ r
    xc = restate_vcycle(As, Ps, Rs, Ds, meshes_n, ip, vtype, lu, bc, None, True, npre, npost, cycle, level + 1)
    if cycle == "W" and level + 1 < len(As) - 1:
        xc = restate_vcycle(As, Ps, Rs, Ds, meshes_n, ip, vtype, lu, bc, xc, False, npre, npost, cycle, level + 1)
    x = x + Ps[level] @ xc
    return restate_relax(As[level], x, b, Ds[level], npost, meshes_n[level], ip, vtype)


def restate_solve(param, b, maxIter, cycle="V", vtype=FULL_VANKA_RB):
    """solveMG's loop (SolveFuncs.jl:3-39) on the hierarchy of `param` from x = 0: (x, [||r_0||, ||r_1||, ...])."""
    ip = param.transferOperatorType == "SystemsFacesMixedLinear"
    ns = [list(map(int, m.n)) for m in param.Meshes]
    lu = spla.splu(sp.csc_matrix(param.As[-1]))
    x = np.zeros_like(b)
    res = [np.linalg.norm(b)]
    for it in range(maxIter):
        x = restate_vcycle(param.As, param.Ps, param.Rs, param.relaxPrecs, ns, ip, vtype, lu, b, x, it == 0,
                           param.relaxPre(1), param.relaxPost(1), cycle)
        res.append(np.linalg.norm(b - param.As[0] @ x))
    return x, np.array(res)


# ---- the fixture's cases: name -> (n, includePressure, complex, seed) ----------------------------------------------------
REF_CASES = {
    "m64": ([6, 4], True, False, 11),
    "f57": ([5, 7], False, False, 12),
    "m435": ([4, 3, 5], True, False, 13),
    "m64c": ([6, 4], True, True, 14),
    "m435c": ([4, 3, 5], True, True, 15),
    "f57c": ([5, 7], False, True, 16),
}
REF_W = 0.6
REF_OMEGA = 0.8


def ref_inputs(mg, name, vtype=FULL_VANKA_RB, w=REF_W):
    n, ip, cx, seed = REF_CASES[name]
    A = mixed_operator(n, ip, omega=REF_OMEGA if cx else None)
    N = A.shape[0]
    x0 = seeded(N, seed, cx)
    b = seeded(N, seed + 100, cx)
    D = mg.setupVankaFacesPreconditioner(A, np.asarray(n), w, ip, vtype)
    return A, x0, b, D
