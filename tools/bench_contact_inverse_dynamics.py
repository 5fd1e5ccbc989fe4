#!/usr/bin/env python3
"""Cost of the contact inverse-dynamics kernel against plain inverse dynamics
and against the composition that gives the same result without it.

The Atlas without ground (33 dofs, 35 bodies, no collision pairs), 1024 worlds
at random states, contact bodies l_foot and r_foot, no guesses, through the
DeviceWorld wrappers with the inputs resident on the device, timed with HIP
events around `--iters` calls of each variant after `--warmup` of the same, in
one process on the same inputs, `--repeats` interleaved rounds of all:

    cid        nimble_contact_inverse_dynamics (one launch)
    id_fwd     (a) nimble_inverse_dynamics, tau only: the floor -- the new
               kernel does this work plus the 6 x 6 solve and the second sweep
    compose_n  (b) what a user needs without the new entry point: inverse
               dynamics; nimble_inverse_dynamics_backward on batch x n items
               with unit grad_tau, whose body-frame grad_wrench is minus the
               bodies' Jacobians; the weighted 6 x 6 solve with torch.linalg;
               inverse dynamics again with the wrenches
    compose_6  the same with only the six root rows of the Jacobians
               (batch x 6 backward items): all the wrenches need, the leanest
               composition

The expanded inputs of the backward launches are prepared outside the timed
region, in the compositions' favour.  The JSON line reports the per-round
means in ms and, for the worst pairing over the rounds, cid / id_fwd and
cid / compose_*; `faster_than_composition_in_every_pairing` is the condition.
It also checks once that cid and compose_n agree.  There is no CPU path:
without a HIP device the tool fails.  Run it under a time limit, as every GPU
step.
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
from nimblephysics_amd.contact_inverse_dynamics import contact_body_indices  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_contact_inverse_dynamics: no HIP device (there is no CPU path)")
    d = torch.device("cuda:0")
    world = workloads.atlas_world(False)
    skel = world.getSkeleton(0)
    bodies = contact_body_indices(world, [skel.getBodyNode("l_foot"), skel.getBodyNode("r_foot")])
    k = len(bodies)
    dev = world.native(d)
    B, n, nb = args.batch, dev.n, dev.nb
    r0 = 0
    st, _ = workloads.random_states(world, B, seed=args.seed, q_scale=0.2, v_scale=0.3)
    rng = np.random.default_rng(args.seed)
    ts = torch.tensor(st, device=d)
    ta = torch.tensor(3.0 * rng.standard_normal((B, n)), device=d)
    tau, full = torch.empty_like(ta), torch.empty_like(ta)
    F = torch.empty((B, k, 6), dtype=torch.float64, device=d)
    stream = torch.cuda.current_stream(d).cuda_stream
    w = torch.tensor([1.0, 1.0, 1.0, 100.0, 100.0, 100.0], dtype=torch.float64, device=d).repeat(k)
    body_idx = torch.tensor(bodies, device=d)

    def expanded(rows):
        """Inputs of a backward launch with one item per (world, row)."""
        g = torch.zeros((B, len(rows), n), dtype=torch.float64, device=d)
        for i, j in enumerate(rows):
            g[:, i, j] = 1.0
        R = len(rows)
        return (ts.repeat_interleave(R, 0).contiguous(), ta.repeat_interleave(R, 0).contiguous(),
                g.reshape(B * R, n).contiguous(), torch.zeros((B * R, nb, 6), dtype=torch.float64, device=d),
                torch.empty((B * R, 2 * n), dtype=torch.float64, device=d),
                torch.empty((B * R, n), dtype=torch.float64, device=d),
                torch.empty((B * R, nb, 6), dtype=torch.float64, device=d))

    root_rows = list(range(r0, r0 + 6))
    ex = {"compose_n": (list(range(n)), expanded(list(range(n)))), "compose_6": (root_rows, expanded(root_rows))}
    tau2 = torch.empty_like(ta)
    F2 = torch.empty_like(F)

    def compose(name):
        rows, (st2, a2, g2, z2, gs2, ga2, gw2) = ex[name]
        dev.inverse_dynamics(ts, ta, full, stream)
        dev.inverse_dynamics_backward(st2, a2, g2, gs2, ga2, stream, body_wrench=z2, wrench_frame="body",
                                      grad_wrench=gw2)
        # J_i[:, row] = -grad_wrench[row, body i]; the root columns, stacked [B, 6k, 6]
        cols = [rows.index(j) for j in root_rows]
        Jr = -gw2.reshape(B, len(rows), nb, 6)[:, cols][:, :, body_idx]  # [B, 6 (col), k, 6 (row)]
        Jr = Jr.permute(0, 2, 3, 1).reshape(B, 6 * k, 6)
        WJ = w[None, :, None] * Jr
        y = torch.linalg.solve(Jr.transpose(1, 2) @ WJ, full[:, r0:r0 + 6].unsqueeze(-1))
        Fc = (WJ @ y).reshape(B, k, 6)
        bw = torch.zeros((B, nb, 6), dtype=torch.float64, device=d)
        bw[:, body_idx] = Fc
        dev.inverse_dynamics(ts, ta, tau2, stream, body_wrench=bw, wrench_frame="body")
        tau2[:, r0:r0 + 6] = 0.0
        F2.copy_(Fc)

    variants = {
        "cid": lambda: dev.contact_inverse_dynamics(ts, ta, bodies, tau, F, stream),
        "id_fwd": lambda: dev.inverse_dynamics(ts, ta, full, stream),
        "compose_n": lambda: compose("compose_n"),
        "compose_6": lambda: compose("compose_6"),
    }

    def run(call, iters, timed):
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(iters)]
        for e in ev:
            e[0].record()
            call()
            e[1].record()
        # one synchronise per window: the queue stays full, so the events
        # bracket device time and not the host's launch latency
        torch.cuda.synchronize()
        if not timed or not ev:
            return 0.0
        return sum(e[0].elapsed_time(e[1]) for e in ev) / iters

    rows = {name: [] for name in variants}
    for call in variants.values():
        run(call, args.warmup, False)
    # the composition computes what the kernel computes
    variants["cid"]()
    variants["compose_n"]()
    torch.cuda.synchronize()
    agree = {"tau": float((tau - tau2).abs().max() / tau.abs().max()), "F": float((F - F2).abs().max() / F.abs().max())}
    for _ in range(args.repeats):
        for name, call in variants.items():
            run(call, 2, False)
            rows[name].append(round(run(call, args.iters, True), 5))
    out = {"tool": "bench_contact_inverse_dynamics", "workload": "atlas without ground, l_foot + r_foot", "batch": B,
           "iters": args.iters, "warmup": args.warmup, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "cid_vs_composition_max_rel_diff": agree}
    for name, r in rows.items():
        out[name] = {"ms": r, "ms_mean": round(float(np.mean(r)), 5)}
    # every pairing of a round of the new kernel with a round of the other
    for other in ("id_fwd", "compose_n", "compose_6"):
        out["cid"]["worst_vs_" + other] = round(max(rows["cid"]) / min(rows[other]), 4)
    out["cid"]["faster_than_composition_in_every_pairing"] = bool(
        max(rows["cid"]) < min(min(rows["compose_n"]), min(rows["compose_6"])))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
