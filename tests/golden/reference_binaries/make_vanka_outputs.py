"""Regenerates vanka_outputs.npz beside this file: the Julia serial schedule of RelaxVankaFacesColor (Vanka.jl:383-425) driven
through the reference's compiled primitives - getVankaVariablesOfCell, cs2loc, computeResidualAtIdx_{FP64,CFP64}_INT64 and
updateSolution_{FP64,CFP64} of deps/src/Vanka.c, built with the flags of deps/build.jl into a temporary directory outside the
repository - for every case of tests/vanka_cases.py::REF_CASES.  Stored per case: the seed, the index lists and x after one
iteration and after two more.  Run from the repository root with the reference tree at hand:
    python tests/golden/reference_binaries/make_vanka_outputs.py /path/to/reference"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multigrid_jl_amd as mg  # noqa: E402
import vanka_cases as V  # noqa: E402

_ll = C.c_longlong
_lp = C.POINTER(_ll)
_vp = C.c_void_p


def _p(a):
    return a.ctypes.data_as(_vp)


def run_case(lib, name):
    n, ip, cx, seed = V.REF_CASES[name]
    A, x0, b, D = V.ref_inputs(mg, name)
    dim = len(n)
    bs, nf = V.block_size(n, ip)
    nn = np.asarray(n, dtype=np.int64)
    nff = np.asarray(nf, dtype=np.int64)
    cells = int(np.prod(n))
    rowptr = np.ascontiguousarray(A.indptr, dtype=np.int64) + 1
    colA = np.ascontiguousarray(A.indices, dtype=np.int64) + 1
    valA = np.ascontiguousarray(np.conj(A.data))          # AT.nzval: the primitive conjugates it back
    resid = lib.computeResidualAtIdx_CFP64_INT64 if cx else lib.computeResidualAtIdx_FP64_INT64
    update = lib.updateSolution_CFP64 if cx else lib.updateSolution_FP64
    Dc = np.asfortranarray(D)
    loc = np.zeros(dim, dtype=np.int64)
    Idxs = np.zeros(bs, dtype=np.int64)
    idx_all = np.zeros((cells, bs), dtype=np.int64)
    colour = np.zeros(cells, dtype=np.int64)
    for i in range(1, cells + 1):
        lib.cs2loc(_ll(i), _p(nn), _ll(dim), _p(loc))
        lib.getVankaVariablesOfCell(_p(loc), _p(nn), _p(nff), _p(Idxs), _ll(1 if ip else 0), _ll(dim))
        idx_all[i - 1] = Idxs
        colour[i - 1] = V.cell_color(list(loc))           # the Julia cellColor (Vanka.c's is the red-black one of the dead path)
    r = np.zeros(bs, dtype=x0.dtype)

    def relax(x, numit):
        y = x.copy()
        for _ in range(numit):
            for c in range(1, 2 ** dim + 1):
                y[:] = x
                for i in np.nonzero(colour == c)[0]:
                    I = np.ascontiguousarray(idx_all[i])
                    resid(_p(rowptr), _p(valA), _p(colA), _p(b), _p(y), _p(I), _p(r), _ll(bs))
                    blk = np.ascontiguousarray(Dc[:, i])
                    update(_p(blk), _p(x), _p(r), C.c_int(bs), _p(I))
        return x

    x1 = relax(x0.copy(), 1)
    x3 = relax(x1.copy(), 2)
    return {f"{name}_seed": np.int64(seed), f"{name}_idx": idx_all, f"{name}_x1": x1, f"{name}_x3": x3}


if __name__ == "__main__":
    ref = sys.argv[1]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "Vanka.so")
        subprocess.check_call(["gcc", "-O3", "-fPIC", "-cpp", "-fopenmp", "-shared", os.path.join(ref, "deps", "src", "Vanka.c"), "-o", so])
        lib = C.CDLL(so)
        for name in V.REF_CASES:
            out.update(run_case(lib, name))
    np.savez_compressed(V.GOLDEN, **out)
    print("wrote", V.GOLDEN, os.path.getsize(V.GOLDEN), "bytes")
