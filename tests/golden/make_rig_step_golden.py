"""Records, for the contact cases of tests/test_wave_emu.py::test_rig_step_emulated,
whether the reference's own compiled dSolveLCP (oracle/_ref/libodelcp.so)
gives both outcomes on the world's LCP under 1e-15-relative symmetric
perturbations of A (oracle.ref_dantzig_ambiguous), into
tests/golden/rig_step_ambiguous.json -- so that the test does not need the
compiled reference solver.  Run from the repo root where oracle/_ref is built
(`make -C oracle ref`).

Each entry holds the LCP (A, b, lo, hi, findex) the verdict was recorded for;
the test compares its own problem with it before it relies on the verdict.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import models  # noqa: E402
from oracle import oracle as O  # noqa: E402


def _enc(v):
    return ["inf" if x == np.inf else "-inf" if x == -np.inf else float(x) for x in np.asarray(v).reshape(-1)]


def main():
    if O.ref_lib() is None:
        raise SystemExit("oracle/_ref/libodelcp.so missing: build with `make -C oracle ref`")
    out = {"source": "oracle.ref_dantzig_ambiguous (the reference's dSolveLCP, dart/external/odelcpsolver/lcp.cpp, "
                     "via oracle/_ref) on the LCPs of test_rig_step_emulated's contact cases, seed = world index",
           "cases": {}}
    for rig, (make, states) in {"ball": (models.ball_world, models.ball_states),
                                "compound": (models.compound_world, models.compound_states)}.items():
        world = make(ground=True)
        st, f = states(8, seed=21, contact=True)
        st, f = st[:2], f[:2]
        ow = O.OracleWorld(world)
        ow.forward(st, f)
        for i in range(2):
            A, bb, lo, hi, fi = O.lcp_problem(ow, i)
            amb = O.ref_dantzig_ambiguous(A, bb, lo, hi, fi, seed=i)
            out["cases"][f"{rig}/{i}"] = {"m": len(bb), "A": _enc(A), "b": _enc(bb), "lo": _enc(lo), "hi": _enc(hi),
                                          "findex": [int(v) for v in fi], "ambiguous": bool(amb)}
            print(rig, i, len(bb), amb)
    with open(os.path.join(HERE, "rig_step_ambiguous.json"), "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
