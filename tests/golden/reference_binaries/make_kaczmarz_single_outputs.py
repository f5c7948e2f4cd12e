"""Regenerates kaczmarz_single_outputs.npz beside this file: what the reference's compiled applyHybridKaczmarz_FP32_INT64 and
applyHybridKaczmarz_CFP32_INT64 (oracle/_ref/parRelax.so, built by oracle/Makefile from the reference tree) return with
numCores = 1, from each case's non-zero start, for every (case, type) pair of tests/kaczmarz_single_cases.py.  Outputs
only: the inputs are generated from seeds.  Run from the repository root after the build:
    python tests/golden/reference_binaries/make_kaczmarz_single_outputs.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multigrid_jl_amd as mg  # noqa: E402
from kaczmarz_single_cases import GOLDEN, PAIRS, run_reference_case  # noqa: E402

if __name__ == "__main__":
    out = {f"{name}_{t}": run_reference_case(mg, name, t) for name, t in PAIRS}
    assert all(np.isfinite(v).all() for v in out.values())
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, {k: (v.shape, str(v.dtype)) for k, v in out.items()}, os.path.getsize(GOLDEN), "bytes")
