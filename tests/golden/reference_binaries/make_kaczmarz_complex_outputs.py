"""Regenerates kaczmarz_complex_outputs.npz beside this file: what the reference's compiled applyHybridKaczmarz_CFP64_INT64
(oracle/_ref/parRelax.so, built by oracle/Makefile from the reference tree) returns with numCores = 1, from x = 0, for every
case of tests/kaczmarz_complex_cases.py::CASES.  Run from the repository root after the build:
    python tests/golden/reference_binaries/make_kaczmarz_complex_outputs.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multigrid_jl_amd as mg  # noqa: E402
from kaczmarz_complex_cases import CASES, GOLDEN, run_reference_case  # noqa: E402

if __name__ == "__main__":
    out = {name: run_reference_case(mg, name) for name in CASES}
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, {k: v.shape for k, v in out.items()})
