#!/usr/bin/env python3
"""Cost of external body wrenches (body_wrench, the `_ext` entry points)
against the shared-model path.

Forward + backward of the box-foot Atlas bench batch (1024 worlds, the bench
sampler's states) through the DeviceWorld wrappers, inputs resident on the
device, timed with HIP events around `--iters` forward and backward launches
after `--warmup` of the same; every launch starts from the same state and a
fresh copy of the same LCP warm-start cache, so the variants do the same work
each iteration:

    shared       nimble_forward / nimble_backward
    ext_zero     the _ext entry points with all-zero wrenches (body frame) and
                 grad_wrench written: the same step and gradients as shared,
                 so the difference is the cost of the path itself (the
                 per-world parameter reads it is built on, the wrench reads
                 and transform, the grad_wrench stores)
    ext_random   the _ext entry points with random wrenches on every body,
                 forces about m_b |g| (body frame): contact sets are the same
                 but the LCPs differ, so this one has no expectation

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
        raise SystemExit("bench_body_wrench: no HIP device (there is no CPU path)")
    d = torch.device("cuda:0")
    world = workloads.atlas_world(True)
    world.setStatusPolicy("record")
    dev = world.native(d)
    B = args.batch
    st, f = workloads.atlas_states(world, B, args.seed)
    g = np.random.default_rng(args.seed).standard_normal(st.shape)
    ts, tf, tg = torch.tensor(st, device=d), torch.tensor(f, device=d), torch.tensor(g, device=d)
    mg = np.maximum(world._body_inertia_base()[:, 0], 0.5) * np.linalg.norm(world.getGravity())
    W = np.random.default_rng(args.seed + 1).standard_normal((B, dev.nb, 6)) * mg[None, :, None]
    W[:, :, :3] *= 0.1  # torques: the forces on a 0.1 m arm
    variants = {
        "shared": None,
        "ext_zero": torch.zeros((B, dev.nb, 6), dtype=torch.float64, device=d),
        "ext_random": torch.tensor(W, device=d),
    }
    gw = torch.empty((B, dev.nb, 6), dtype=torch.float64, device=d)
    cache0 = torch.zeros((B, dev.cache_doubles), dtype=torch.float64, device=d)
    cache0[:, 0] = -1
    cache = cache0.clone()
    nxt = torch.empty_like(ts)
    snap = torch.zeros((B, dev.snapshot_doubles), dtype=torch.float64, device=d)
    gs, gf = torch.empty_like(ts), torch.empty_like(tf)
    stream = torch.cuda.current_stream(d).cuda_stream

    def run(bw, iters, timed):
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters)]
        for e in ev:
            cache.copy_(cache0)
            e[0].record()
            if bw is None:
                dev.forward(ts, tf, cache, nxt, snap, stream)
            else:
                dev.forward(ts, tf, cache, nxt, snap, stream, body_wrench=bw, wrench_frame="body")
            e[1].record()
            if bw is None:
                dev.backward(ts, tf, snap, tg, gs, gf, stream)
            else:
                dev.backward(ts, tf, snap, tg, gs, gf, stream, body_wrench=bw, wrench_frame="body", grad_wrench=gw)
            e[2].record()
        # one synchronise per window: the queue stays full, so the events
        # bracket kernel time and not the host's launch latency
        torch.cuda.synchronize()
        if not timed or not ev:
            return 0.0, 0.0
        return (sum(e[0].elapsed_time(e[1]) for e in ev) / iters, sum(e[1].elapsed_time(e[2]) for e in ev) / iters)

    rows = {k: {"fwd_ms": [], "bwd_ms": []} for k in variants}
    for bw in variants.values():
        run(bw, args.warmup, False)
    for _ in range(args.repeats):
        for name, bw in variants.items():
            run(bw, 2, False)
            fwd, bwd = run(bw, args.iters, True)
            rows[name]["fwd_ms"].append(round(fwd, 5))
            rows[name]["bwd_ms"].append(round(bwd, 5))
    out = {"tool": "bench_body_wrench", "workload": "atlas (box feet)", "batch": B, "iters": args.iters,
           "warmup": args.warmup, "repeats": args.repeats, "device": torch.cuda.get_device_name(0)}
    for name, r in rows.items():
        tot = [a + b for a, b in zip(r["fwd_ms"], r["bwd_ms"])]
        out[name] = {"fwd_ms": r["fwd_ms"], "bwd_ms": r["bwd_ms"],
                     "fwd_ms_mean": round(float(np.mean(r["fwd_ms"])), 5),
                     "bwd_ms_mean": round(float(np.mean(r["bwd_ms"])), 5),
                     "fwd_bwd_ms_range": [round(min(tot), 5), round(max(tot), 5)]}
    base = out["shared"]["fwd_ms_mean"] + out["shared"]["bwd_ms_mean"]
    for name in ("ext_zero", "ext_random"):
        out[name]["vs_shared"] = round((out[name]["fwd_ms_mean"] + out[name]["bwd_ms_mean"]) / base, 4)
        out[name]["fwd_vs_shared"] = round(out[name]["fwd_ms_mean"] / out["shared"]["fwd_ms_mean"], 4)
        out[name]["bwd_vs_shared"] = round(out[name]["bwd_ms_mean"] / out["shared"]["bwd_ms_mean"], 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
