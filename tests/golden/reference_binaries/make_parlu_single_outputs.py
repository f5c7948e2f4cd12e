"""Regenerates parlu_single_outputs.npz beside this file: what the reference's compiled applyLUsolve_FP32_UINT32,
applyLUsolve_CFP32_UINT32 and applyLUsolve_CFP32_INT64 (oracle/_ref/parLU.so, built by oracle/Makefile from the reference
tree) return for the cases of tests/parlu_single_cases.py::pinned_cases - plain and adjoint solves, one and several
right-hand sides, on the matrices stored in parlu_complex_outputs.npz.  Data only.  Run from the repository root after the
build:
    python tests/golden/reference_binaries/make_parlu_single_outputs.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from parlu_single_cases import GOLDEN, case, err, pinned_cases, ref_lu_solve_single  # noqa: E402

if __name__ == "__main__":
    out = {}
    for form, nrhs, t in pinned_cases():
        name, F, B, E = case(form, nrhs, t)
        X = ref_lu_solve_single(F, B, form, t)
        print(f"{name}: err(reference) {err(X, E):.2e}")
        out[name] = X
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN)
