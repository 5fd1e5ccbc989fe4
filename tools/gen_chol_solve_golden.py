"""Record the outputs tests/test_gpu_chol_solve.py pins: next state, grad_state
and grad_action of nimble.timestep forward + backward on the cases of
tests/chol_solve_cases.py, from the library NIMBLE_AMD_LIB names (or the
built one).  Run once on the GPU with the library of the commit *before* a
change to the Cholesky solves, so that the test holds the change to that
commit's bits:

    NIMBLE_AMD_LIB=<that commit's libnimble_amd.so> python tools/gen_chol_solve_golden.py [out.npz]

Writes tests/golden/chol_solve_parent.npz by default (a few tens of KB).
The Atlas seed (chol_solve_cases.ATLAS_SEED) was picked with the CPU oracle's
clamping counts (oracle.lcp_flags) over seeds 1000..1011: 1008 has four
clamping and four contact-free worlds in both steps.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import chol_solve_cases as cases  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "chol_solve_parent.npz")
    rec = {}
    for name, (world, st, f, steps) in cases.cases().items():
        res = cases.run(world, st, f, steps)
        if name == "atlas":
            counts = cases.atlas_counts(res)
            print("atlas (clamping, contact-free) per step:", counts)
            for clamping, free in counts:
                assert clamping >= cases.MIN_WORLDS, "too few clamping worlds: the batched solves would go untested"
                assert free >= cases.MIN_WORLDS, "too few contact-free worlds: the two-column solve would go untested"
        for k, v in res.items():
            assert np.isfinite(v).all(), (name, k)
            rec[f"{name}/{k}"] = v
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
