"""The inverse-dynamics kernels on the CPU: nimble_inverse_dynamics_kernel and
nimble_inverse_dynamics_backward_kernel compiled for the host with
AddressSanitizer against the emulated wavefront (tests/cpp/wave_emu,
invdyn_emu.cpp; the host build of timestep.hip takes every kernel set) and run
through the emulated C ABI on the cartpole (with damping, stiffness and rest
positions) and on the ball rig without ground, B = 2: tau, mass_matrix, bias,
grad_state and grad_ddq against the oracle references of invdyn_refs.py
(values from oracle_mass_matrix / oracle_coriolis_gravity, gradients from the
oracle's analytic step Jacobian), and any out-of-bounds access aborts the run.
The run with wrenches (both frames) is held to the identity that ties its
outputs together: tau is linear in the wrench with d tau / dW = -(body twist
per unit rate), so g . (tau(W) - tau(0)) = sum_b grad_wrench_b . W_b.

Only these two small models: an Atlas-sized emulator case takes tens of
minutes.  No GPU needed.

Results before this feature: FEATURE MISSING -- tests/cpp/wave_emu/invdyn_emu.cpp
and the C-ABI entry points it calls do not exist, so every test here fails on
the parent commit.

Observed maxima under _rel (floor 1e-5), bar RTOL = 1e-6, cartpole / ball
rig: tau 5.2e-16 / 5.5e-13, mass_matrix 1.8e-16 / 1.2e-12, bias 3.5e-14 /
3.7e-13, grad_state 4.8e-14 / 3.0e-11, grad_ddq 2.2e-16 / 8.3e-13; the wrench
identity to 1.0e-15 / 2.8e-16 relative.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import invdyn_refs
import models
import wave_emu
from test_gpu_contact_parity import RTOL, _rel

pytestmark = pytest.mark.skipif(not os.path.exists(wave_emu.CLANG) or shutil.which("true") is None,
                                reason="needs the ROCm clang for the host build")


def _cartpole():
    w = invdyn_refs.damped_cartpole()
    st, _ = models.random_states(w, 2, seed=3, q_scale=0.5, v_scale=1.0)
    return w, st


def _ball():
    w = models.ball_world(ground=False)
    st, _ = models.ball_states(2, seed=21, contact=False)
    return w, st


def _run(world, st, a, g, frame, wrench):
    exe = wave_emu.build("invdyn_emu")
    lines = invdyn_refs.desc_lines(world)
    f = wave_emu._fmt
    lines += [str(st.shape[0]), f(st), f(a), f(g), str(frame), f(wrench)]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], input="\n".join(lines), capture_output=True, text=True, timeout=1800, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    out = {}
    for ln in r.stdout.splitlines():
        t = ln.split()
        out[t[0]] = np.array([float(x) for x in t[1:]])
    return out


@pytest.mark.parametrize("name,frame", [("cartpole", 0), ("ball", 1)])
def test_inverse_dynamics_emulated(name, frame):
    world, st = {"cartpole": _cartpole, "ball": _ball}[name]()
    B, n = st.shape[0], world.getNumDofs()
    nb = int(world.desc_arrays()["num_bodies"])
    a = invdyn_refs.accelerations((B, n), seed=5)
    g = np.random.default_rng(6).standard_normal((B, n))
    W = np.random.default_rng(7).standard_normal((B, nb, 6))
    out = _run(world, st, a, g, frame, W)
    ref = invdyn_refs.Ref(world)
    tau = out["tau"].reshape(B, n)
    e = {"tau": _rel(tau, ref.tau_batch(st, a))}
    mm, bias = out["mm"].reshape(B, n, n), out["bias"].reshape(B, n)
    e["mass_matrix"] = max(_rel(mm[b], ref.o.mass_matrix(st[b, :n])) for b in range(B))
    e["bias"] = max(_rel(bias[b], ref.o.coriolis_gravity(st[b, :n], st[b, n:])) for b in range(B))
    gs, ga = out["gs"].reshape(B, 2 * n), out["ga"].reshape(B, n)
    rgs, rga = np.zeros_like(gs), np.zeros_like(ga)
    for b in range(B):
        dq, dv, da = ref.analytic(st[b, :n], st[b, n:], a[b])
        rgs[b] = np.concatenate([dq.T @ g[b], dv.T @ g[b]])
        rga[b] = da.T @ g[b]
    e["grad_state"] = _rel(gs, rgs)
    e["grad_ddq"] = _rel(ga, rga)
    # with wrenches: linear in them, through minus the body twists
    tauw, gw = out["tauw"].reshape(B, n), out["gw"].reshape(B, nb, 6)
    lhs = np.einsum("bi,bi->b", g, tauw - tau)
    rhs = np.einsum("bkj,bkj->b", gw, W)
    e["wrench identity"] = float((np.abs(lhs - rhs) / np.abs(rhs)).max())
    # M g does not see the wrench
    e["grad_ddq (wrench)"] = _rel(out["gaw"].reshape(B, n), rga)
    print(name, {k: f"{v:.2e}" for k, v in e.items()})
    assert np.abs(rhs).min() > 1e-3
    for k, v in e.items():
        assert v <= RTOL, (name, k, v)
    # tau_ext depends on q (through the S_k, and a body-frame wrench itself)
    # and not on v
    gsw = out["gsw"].reshape(B, 2 * n)
    assert np.abs(gsw[:, :n] - gs[:, :n]).max() > 1e-6
    assert _rel(gsw[:, n:], rgs[:, n:]) <= RTOL
