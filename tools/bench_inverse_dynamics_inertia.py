#!/usr/bin/env python3
"""Cost of the inverse dynamics' gradient and Jacobian in the inertial
parameters.

The Atlas without ground (33 dofs, 34 bodies, no collision pairs), 1024 worlds
at random states, each world on its own parameter rows (the model's values
scaled by 0.9 .. 1.1 per world), through the DeviceWorld wrappers with the
inputs resident on the device, timed with HIP events around `--iters` launches
of each kernel after `--warmup` of the same, in one process on the same inputs:

    id_bwd          nimble_inverse_dynamics_backward   (grad_state, grad_ddq)
    id_bwd_inertia  nimble_invdyn_backward_inertia     (the same and grad_inertia)
    id_jacobian     nimble_invdyn_inertia_jacobian     (d tau / d theta, [B, n, nb, 10])
    id_fwd_pw       nimble_inverse_dynamics            (tau, per-world parameters)
    fd_jacobian     20 nb launches of id_fwd_pw: what the matrix costs without
                    the kernel, by central differences through the existing
                    forward (two evaluations per parameter; forming the
                    perturbed arrays and the differences is not counted);
                    `--fd-iters` timed repetitions

(a) the gradient's cost on top of the backward it rides on: id_bwd_inertia
against id_bwd, expected to be a small fraction since only lane = body work
is added; (b) the Jacobian kernel against the finite-difference route.  The
JSON line reports the per-round means in ms over `--repeats` interleaved
rounds and, for both, the ratio of the means and the worst pairing of rounds.
There is no CPU path: without a HIP device the tool fails.
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
    ap.add_argument("--fd-iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_inverse_dynamics_inertia: no HIP device (there is no CPU path)")
    d = torch.device("cuda:0")
    world = workloads.atlas_world(False)
    dev = world.native(d)
    B, n, nb = args.batch, dev.n, dev.nb
    st, _ = workloads.random_states(world, B, seed=args.seed, q_scale=0.2, v_scale=0.3)
    rng = np.random.default_rng(args.seed)
    ts = torch.tensor(st, device=d)
    ta = torch.tensor(3.0 * rng.standard_normal((B, n)), device=d)
    tg = torch.tensor(rng.standard_normal((B, n)), device=d)
    bi = torch.tensor(world._body_inertia_base()[None] * rng.uniform(0.9, 1.1, (B, 1, 1)), device=d).contiguous()
    gs, ga, tau = torch.empty_like(ts), torch.empty_like(ta), torch.empty_like(ta)
    gi = torch.empty((B, nb, 10), dtype=torch.float64, device=d)
    J = torch.empty((B, n, nb, 10), dtype=torch.float64, device=d)
    stream = torch.cuda.current_stream(d).cuda_stream
    fd_launches = 20 * nb

    def fd():
        for _ in range(fd_launches):
            dev.inverse_dynamics(ts, ta, tau, stream, body_inertia=bi)

    variants = {
        "id_bwd": (lambda: dev.inverse_dynamics_backward(ts, ta, tg, gs, ga, stream, body_inertia=bi), args.iters),
        "id_bwd_inertia": (lambda: dev.inverse_dynamics_backward(ts, ta, tg, gs, ga, stream, body_inertia=bi,
                                                                 grad_inertia=gi), args.iters),
        "id_jacobian": (lambda: dev.inverse_dynamics_inertia_jacobian(ts, ta, J, stream, body_inertia=bi),
                        args.iters),
        "id_fwd_pw": (lambda: dev.inverse_dynamics(ts, ta, tau, stream, body_inertia=bi), args.iters),
        "fd_jacobian": (fd, args.fd_iters),
    }

    def run(call, iters, timed):
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(iters)]
        for e in ev:
            e[0].record()
            call()
            e[1].record()
        # one synchronise per window: the queue stays full, so the events
        # bracket kernel time and not the host's launch latency
        torch.cuda.synchronize()
        if not timed or not ev:
            return 0.0
        return sum(e[0].elapsed_time(e[1]) for e in ev) / iters

    rows = {k: [] for k in variants}
    for name, (call, iters) in variants.items():
        run(call, 1 if name == "fd_jacobian" else args.warmup, False)
    for _ in range(args.repeats):
        for name, (call, iters) in variants.items():
            if name != "fd_jacobian":
                run(call, 2, False)
            rows[name].append(round(run(call, iters, True), 5))
    out = {"tool": "bench_inverse_dynamics_inertia", "workload": "atlas without ground", "batch": B, "dofs": n,
           "bodies": nb, "iters": args.iters, "fd_iters": args.fd_iters, "fd_launches": fd_launches,
           "warmup": args.warmup, "repeats": args.repeats, "device": torch.cuda.get_device_name(0)}
    for name, r in rows.items():
        out[name] = {"ms": r, "ms_mean": round(float(np.mean(r)), 5)}
    for mine, theirs in (("id_bwd_inertia", "id_bwd"), ("id_jacobian", "fd_jacobian")):
        out[mine]["mean_vs_" + theirs] = round(float(np.mean(rows[mine]) / np.mean(rows[theirs])), 6)
        out[mine]["worst_vs_" + theirs] = round(max(rows[mine]) / min(rows[theirs]), 6)
    out["jacobian_bytes"] = int(J.numel() * 8)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
