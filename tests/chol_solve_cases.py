"""The cases of tests/test_gpu_chol_solve.py and of the generator of its
recorded outputs (tools/gen_chol_solve_golden.py): small batches whose step
goes through every instance of the solves with the mass matrix's Cholesky
factor (csrc/chol_wave.cuh), run through nimble.timestep forward + backward
with a seeded upstream gradient.

  cartpole     B = 4      n = 2: no full block of eight substitution steps
  kr5_ground   B = 4      n = 6, the KR5 arm with the ground skeleton
  atlas        B = 8      n = 33 (four blocks and one single step), two
                          consecutive steps of workloads.atlas_states with
                          the LCP warm start carried over; ATLAS_SEED makes
                          the batch hold clamping worlds (the backward's two
                          batched solves, 5 and 4 columns) and contact-free
                          worlds (the two-column solve) in both steps
"""
import numpy as np

from nimblephysics_amd import assets, workloads
from nimblephysics_amd._native import SN_NC

ATLAS_SEED = 1008
GRAD_SEED = 29
MIN_WORLDS = 2  # of each kind, in each Atlas step


def kr5_ground_world():
    w = workloads.kr5_world()
    w.addSkeleton(assets.load_skeleton("kr5_ground"))
    return w


def cases():
    """name -> (world, state [B, 2n], action [B, n], steps)"""
    out = {}
    w = workloads.cartpole_world()
    out["cartpole"] = (w, *workloads.random_states(w, 4, seed=5), 1)
    w = kr5_ground_world()
    out["kr5_ground"] = (w, *workloads.random_states(w, 4, seed=6), 1)
    w = workloads.atlas_world(True)
    out["atlas"] = (w, *workloads.atlas_states(w, 8, ATLAS_SEED), 2)
    return out


def run(world, st, f, steps, device="cuda:0"):
    """Per step: next state, grad_state, grad_action and the clamping-row
    counts of the worlds' snapshot headers, as numpy arrays keyed
    '<what><step>'."""
    import torch
    import nimblephysics_amd as nimble

    world.setStatusPolicy("record")
    g = np.random.default_rng(GRAD_SEED).standard_normal(st.shape)
    tf = torch.tensor(f, device=device)
    out = {}
    for k in range(steps):
        ts = torch.tensor(st, device=device, requires_grad=True)
        ta = tf.clone().requires_grad_(True)
        nxt = nimble.timestep(world, ts, ta)
        nxt.backward(torch.tensor(g, device=device))
        torch.cuda.synchronize()
        out[f"next{k}"] = nxt.detach().cpu().numpy()
        out[f"grad_state{k}"] = ts.grad.cpu().numpy()
        out[f"grad_action{k}"] = ta.grad.cpu().numpy()
        snap = getattr(world, "_last_snapshot", None)
        nc = snap[:, SN_NC].cpu().numpy() if snap is not None and snap.shape[1] > SN_NC else np.zeros(st.shape[0])
        out[f"clamping{k}"] = nc.astype(np.int64)
        st = out[f"next{k}"]
    return out


def atlas_counts(res, steps=2):
    """[(clamping worlds, contact-free worlds)] per Atlas step"""
    return [(int((res[f"clamping{k}"] > 0).sum()), int((res[f"clamping{k}"] == 0).sum())) for k in range(steps)]
