"""Regenerates dd_single_outputs.npz beside this file: the iterates of the single-precision Schwarz sweep by the reference's own
arithmetic for the cases of tests/dd_single_cases.py - the residual term by term in VAL (DDSerial.jl:4-20), every sub-solve by the
reference's compiled applyLUsolve_FP32_UINT32 / _CFP32_UINT32 / _CFP32_INT64 (oracle/_ref/parLU.so, built by oracle/Makefile from
the reference tree), x[I] += t in single - after one sweep from zero and after two more.  Data only: recorded vectors.  It prints
the fixture guard err(reference) <= REF_ERR_MAX for every case.  Run from the repository root after the build:
    python tests/golden/reference_binaries/make_dd_single_outputs.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multigrid_jl_amd as mg  # noqa: E402
from dd_single_cases import CASES, GOLDEN, REF_ERR_MAX, SWEEPS, case, err  # noqa: E402

if __name__ == "__main__":
    out = {}
    for name in CASES:
        c = case(mg, name)
        X, E = c.reference_sweeps(), c.E()
        for s in SWEEPS:
            e = err(X[s], E[s])
            print(f"{name} after {s} sweep(s): err(reference) {e:.2e} {'ok' if e <= REF_ERR_MAX else 'BREAKS THE GUARD'}")
            out[f"{name}_s{s}"] = X[s]
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN)
