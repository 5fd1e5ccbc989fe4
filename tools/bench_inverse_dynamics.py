#!/usr/bin/env python3
"""Cost of the inverse-dynamics kernels against the contact-free step's.

The Atlas without ground (33 dofs, 35 bodies, no collision pairs), 1024 worlds
at random states, through the DeviceWorld wrappers with the inputs resident
on the device, timed with HIP events around `--iters` launches of each kernel
after `--warmup` of the same, in one process on the same inputs:

    step_fwd   nimble_forward   (nimble_forward_kernel: kinematics, composites,
               mass matrix, Cholesky, solve, integration, dynamics cache)
    step_bwd   nimble_backward  (nimble_backward_kernel: cache reload, two
               solves, accelerations, adjoint vectors, per-dof columns)
    id_fwd     nimble_inverse_dynamics           (tau only)
    id_fwd_all nimble_inverse_dynamics           (tau, mass_matrix and bias)
    id_bwd     nimble_inverse_dynamics_backward  (grad_state, grad_ddq)

The inverse-dynamics kernels run a strict subset of the step's work -- no
factorisation, no solves, no snapshot -- so id_fwd must be no slower than
step_fwd and id_bwd no slower than step_bwd in every pairing of the
interleaved rounds (`--repeats` rounds of all five); the JSON line reports
the per-round means in ms, the worst pairing's ratio for each, and the LDS
bytes per workgroup of the four layouts with the worlds per CU they allow
(160 KB of LDS per CU).  There is no CPU path: without a HIP device the tool
fails.
"""
import argparse
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nimblephysics_amd import workloads  # noqa: E402


def _lds_report(world, d):
    """LDS bytes per workgroup of the step's and the inverse-dynamics layouts:
    nimble_world_create's NIMBLE_AMD_VERBOSE report (stderr of the C library)."""
    r, w = os.pipe()
    saved = os.dup(2)
    os.environ["NIMBLE_AMD_VERBOSE"] = "1"
    try:
        sys.stderr.flush()
        os.dup2(w, 2)
        world._version += 1  # (a new handle: the report comes from its creation)
        world.native(d)
    finally:
        os.dup2(saved, 2)
        os.close(w)
        os.close(saved)
        del os.environ["NIMBLE_AMD_VERBOSE"]
    with os.fdopen(r) as fh:
        txt = fh.read()
    out = {}
    m = re.search(r"LDS forward (\d+) B .* backward (\d+) B", txt)
    if m:
        out["step_fwd"], out["step_bwd"] = int(m.group(1)), int(m.group(2))
    m = re.search(r"LDS inverse dynamics (\d+) B, its backward (\d+) B", txt)
    if m:
        out["id_fwd"], out["id_bwd"] = int(m.group(1)), int(m.group(2))
    return out


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
        raise SystemExit("bench_inverse_dynamics: no HIP device (there is no CPU path)")
    d = torch.device("cuda:0")
    world = workloads.atlas_world(False)
    lds = _lds_report(world, d)
    dev = world.native(d)
    B, n = args.batch, dev.n
    st, f = workloads.random_states(world, B, seed=args.seed, q_scale=0.2, v_scale=0.3)
    rng = np.random.default_rng(args.seed)
    ts, tf = torch.tensor(st, device=d), torch.tensor(f, device=d)
    tg = torch.tensor(rng.standard_normal(st.shape), device=d)
    ta = torch.tensor(3.0 * rng.standard_normal((B, n)), device=d)
    tgt = torch.tensor(rng.standard_normal((B, n)), device=d)
    cache = torch.zeros((B, dev.cache_doubles), dtype=torch.float64, device=d)
    cache[:, 0] = -1
    nxt = torch.empty_like(ts)
    snap = torch.zeros((B, dev.snapshot_doubles), dtype=torch.float64, device=d)
    gs, gf = torch.empty_like(ts), torch.empty_like(tf)
    tau, ga = torch.empty_like(ta), torch.empty_like(ta)
    M = torch.empty((B, n, n), dtype=torch.float64, device=d)
    C = torch.empty((B, n), dtype=torch.float64, device=d)
    stream = torch.cuda.current_stream(d).cuda_stream
    dev.forward(ts, tf, cache, nxt, snap, stream)  # (the snapshot step_bwd reads)
    variants = {
        "step_fwd": lambda: dev.forward(ts, tf, cache, nxt, snap, stream),
        "step_bwd": lambda: dev.backward(ts, tf, snap, tg, gs, gf, stream),
        "id_fwd": lambda: dev.inverse_dynamics(ts, ta, tau, stream),
        "id_fwd_all": lambda: dev.inverse_dynamics(ts, ta, tau, stream, mass_matrix=M, bias=C),
        "id_bwd": lambda: dev.inverse_dynamics_backward(ts, ta, tgt, gs, ga, stream),
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
    for call in variants.values():
        run(call, args.warmup, False)
    for _ in range(args.repeats):
        for name, call in variants.items():
            run(call, 2, False)
            rows[name].append(round(run(call, args.iters, True), 5))
    out = {"tool": "bench_inverse_dynamics", "workload": "atlas without ground", "batch": B, "iters": args.iters,
           "warmup": args.warmup, "repeats": args.repeats, "device": torch.cuda.get_device_name(0)}
    for name, r in rows.items():
        out[name] = {"ms": r, "ms_mean": round(float(np.mean(r)), 5)}
    # every pairing of an inverse-dynamics round with a round of its counterpart
    for mine, theirs in (("id_fwd", "step_fwd"), ("id_bwd", "step_bwd")):
        out[mine]["worst_vs_" + theirs] = round(max(rows[mine]) / min(rows[theirs]), 4)
        out[mine]["no_slower_in_every_pairing"] = bool(max(rows[mine]) <= min(rows[theirs]))
    out["lds_bytes"] = lds
    out["worlds_per_cu"] = {k: (160 * 1024) // v for k, v in lds.items() if v > 0}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
