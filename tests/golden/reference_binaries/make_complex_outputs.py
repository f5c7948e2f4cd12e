"""Regenerates complex_outputs.npz beside this file: what the reference's compiled applyLUsolve_CFP64_INT64
(oracle/_ref/parLU.so, built by oracle/Makefile from the reference tree) returns for the inputs of
tests/test_complex_host.py::test_complex_lu_layout_matches_reference_binary.  Run from the repository root after the build:
    python tests/golden/reference_binaries/make_complex_outputs.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from complex_cases import lu_pin_system, ref_lu_solve_complex  # noqa: E402

if __name__ == "__main__":
    so = os.path.join(ROOT, "oracle", "_ref", "parLU.so")
    A, lu, b = lu_pin_system()
    x = ref_lu_solve_complex(so, lu, b)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "complex_outputs.npz")
    np.savez_compressed(out, parlu_complex_helmholtz2d=x)
    print("wrote", out, "residual", np.abs(A @ x - b).max())
