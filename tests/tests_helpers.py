import os

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_binaries", "outputs.npz")


def reference_output(name, binary, call):
    """What the reference's compiled code (oracle/_ref/<binary>, built by oracle/Makefile where the reference tree is present)
    returns for a test's inputs.  Where the binary was built, call() runs it, and its result must match the copy stored
    under `name` in tests/golden/reference_binaries/outputs.npz; elsewhere that stored copy is returned.  Re-record after
    changing a test's inputs, with the binaries built:
        MG_RECORD_REFERENCE=1 python -m pytest tests/test_reference_parlu.py tests/test_reference_parrelax.py"""
    stored = dict(np.load(REFERENCE_GOLDEN)) if os.path.exists(REFERENCE_GOLDEN) else {}
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", binary)):
        assert name in stored, f"{name}: oracle/_ref/{binary} not built and no stored output in {REFERENCE_GOLDEN}"
        return stored[name]
    out = np.asarray(call())
    if os.environ.get("MG_RECORD_REFERENCE") == "1":
        stored[name] = out
        np.savez_compressed(REFERENCE_GOLDEN, **stored)
    else:
        assert name in stored and stored[name].shape == out.shape, f"{name}: no stored output of this shape (re-record it)"
        assert np.abs(out - stored[name]).max() <= 1e-12 * np.abs(out).max(), f"{name}: stored output is stale (re-record it)"
    return out


def divsiggrad(n, shift, seed=42):
    from multigrid_jl_amd.operators import getRegularMesh, getNodalDivSigGradMatrix, entrynorm1
    rng = np.random.default_rng(seed)
    mesh = getRegularMesh([0, 1] * len(n), n)
    m = np.exp(rng.standard_normal(mesh.nc))
    A = getNodalDivSigGradMatrix(mesh, m)
    A = (A + shift * entrynorm1(A) * sp.identity(A.shape[0])).tocsr()
    A.sort_indices()
    return A
