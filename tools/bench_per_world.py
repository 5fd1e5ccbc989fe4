#!/usr/bin/env python3
"""Cost of the per-world body inertial parameters (body_inertia, the `_pw`
entry points) against the shared-model path.

Forward + backward of the box-foot Atlas bench batch (1024 worlds, the bench
sampler's states) through the DeviceWorld wrappers, inputs resident on the
device, timed with HIP events around `--iters` forward and backward launches
after `--warmup` of the same; every launch starts from the same state and a
fresh copy of the same LCP warm-start cache, so the three variants do the
same work each iteration:

    shared       nimble_forward / nimble_backward (the model's parameters)
    pw_model     the _pw entry points, body_inertia = the model's own values
                 in every world (same arithmetic: the cost of the reads)
    pw_sets      the _pw entry points with three parameter sets, world b
                 taking set b % 3 (masses x {1, 0.8, 1.3}, COM shifted by up
                 to 2 cm, diagonal moments x {1, 1.2, 0.7}, off-diagonals of
                 5 % of the smallest diagonal): contact sets are the same but
                 LCP paths may differ, so this one has no expectation

The variants run interleaved, `--repeats` rounds of all three, and one JSON
line reports the per-round mean forward and backward times in ms with their
ranges.  There is no CPU path: without a HIP device the tool fails.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nimblephysics_amd import workloads  # noqa: E402


def parameter_sets(world):
    """The model's [nb, 10] values and the two perturbed sets (see above)."""
    base = world._body_inertia_base()
    sets = [base]
    spec = ((0.8, (0.02, -0.01, 0.005), 1.2, (0.05, 0.0, 0.0)), (1.3, (-0.015, 0.02, -0.02), 0.7, (0.0, -0.05, 0.05)))
    for mass, com, diag, off in spec:
        P = base.copy()
        massive = base[:, 0] > 0
        P[:, 0] *= mass
        P[massive, 1:4] += np.array(com)
        P[:, 4:7] *= diag
        P[:, 7:10] = P[:, 4:7].min(axis=1)[:, None] * np.array(off)
        sets.append(P)
    return sets


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_per_world: no HIP device (there is no CPU path)")
    d = torch.device("cuda:0")
    world = workloads.atlas_world(True)
    world.setStatusPolicy("record")
    dev = world.native(d)
    B = args.batch
    st, f = workloads.atlas_states(world, B, args.seed)
    g = np.random.default_rng(args.seed).standard_normal(st.shape)
    ts, tf, tg = torch.tensor(st, device=d), torch.tensor(f, device=d), torch.tensor(g, device=d)
    sets = parameter_sets(world)
    variants = {
        "shared": None,
        "pw_model": torch.tensor(np.broadcast_to(sets[0], (B,) + sets[0].shape).copy(), device=d),
        "pw_sets": torch.tensor(np.stack([sets[b % 3] for b in range(B)]), device=d),
    }
    cache0 = torch.zeros((B, dev.cache_doubles), dtype=torch.float64, device=d)
    cache0[:, 0] = -1
    cache = cache0.clone()
    nxt = torch.empty_like(ts)
    snap = torch.zeros((B, dev.snapshot_doubles), dtype=torch.float64, device=d)
    gs, gf = torch.empty_like(ts), torch.empty_like(tf)
    stream = torch.cuda.current_stream(d).cuda_stream

    def run(bi, iters, timed):
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters)]
        for e in ev:
            cache.copy_(cache0)
            e[0].record()
            dev.forward(ts, tf, cache, nxt, snap, stream, body_inertia=bi)
            e[1].record()
            dev.backward(ts, tf, snap, tg, gs, gf, stream, body_inertia=bi)
            e[2].record()
        # one synchronise per window: the queue stays full, so the events
        # bracket kernel time and not the host's launch latency
        torch.cuda.synchronize()
        if not timed or not ev:
            return 0.0, 0.0
        return (sum(e[0].elapsed_time(e[1]) for e in ev) / iters, sum(e[1].elapsed_time(e[2]) for e in ev) / iters)

    rows = {k: {"fwd_ms": [], "bwd_ms": []} for k in variants}
    for bi in variants.values():
        run(bi, args.warmup, False)
    for _ in range(args.repeats):
        for name, bi in variants.items():
            run(bi, 2, False)
            fwd, bwd = run(bi, args.iters, True)
            rows[name]["fwd_ms"].append(round(fwd, 5))
            rows[name]["bwd_ms"].append(round(bwd, 5))
    out = {"tool": "bench_per_world", "workload": "atlas (box feet)", "batch": B, "iters": args.iters,
           "warmup": args.warmup, "repeats": args.repeats, "device": torch.cuda.get_device_name(0)}
    for name, r in rows.items():
        tot = [a + b for a, b in zip(r["fwd_ms"], r["bwd_ms"])]
        out[name] = {"fwd_ms": r["fwd_ms"], "bwd_ms": r["bwd_ms"],
                     "fwd_ms_mean": round(float(np.mean(r["fwd_ms"])), 5),
                     "bwd_ms_mean": round(float(np.mean(r["bwd_ms"])), 5),
                     "fwd_bwd_ms_range": [round(min(tot), 5), round(max(tot), 5)]}
    base = out["shared"]["fwd_ms_mean"] + out["shared"]["bwd_ms_mean"]
    for name in ("pw_model", "pw_sets"):
        out[name]["vs_shared"] = round((out[name]["fwd_ms_mean"] + out[name]["bwd_ms_mean"]) / base, 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
