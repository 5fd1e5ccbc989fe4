"""The contact inverse-dynamics kernel on the CPU:
nimble_contact_inverse_dynamics_kernel compiled for the host with
AddressSanitizer against the emulated wavefront (tests/cpp/wave_emu,
contact_invdyn_emu.cpp; the host build of timestep.hip takes every kernel
set) and run through the emulated C ABI on the 12-dof biped rig
(contact_invdyn_refs.rig_world: free root, two revolute legs with welded feet,
an arm on a UniversalJoint, one joint with damping and stiffness), B = 2, with
a known body-frame wrench on every body: k = 1 (left foot), k = 2 without
guesses (both feet) and k = 3 with guesses (feet and the arm, whose
device-model index is shifted by its joint's chain frame).

tau and the contact wrenches are held to the numpy restatement of the
reference's formulas (contact_invdyn_refs.reference: KKT solve / pinv), fed
with tau_full and the bodies' Jacobians from the existing, separately verified
entry points run in the same emulation (nimble_inverse_dynamics, and
nimble_inverse_dynamics_backward with unit grad_tau, whose body-frame
grad_wrench is minus the Jacobian's column); tau_full itself is also held to
the oracle (invdyn_refs.Ref) without the wrench.  The root rows must be
exactly 0, and the linear closure tau_full - tau = J^T F must hold outside
them.  Any out-of-bounds access aborts the run.  No GPU needed.

Results before this feature: FEATURE MISSING -- contact_invdyn_emu.cpp and
the entry point it calls do not exist, so every test here fails on the parent
commit.

Observed maxima under _rel (floor 1e-5), bar RTOL = 1e-6, k = 1 / 2 / 3:
tau_full against the oracle 4.0e-15; closure 8.0e-16 / 1.2e-15 / 5.1e-15; tau 5.3e-14 / 5.9e-14 /
1.7e-14; contact wrenches 5.2e-14 / 1.2e-13 / 5.0e-14.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import contact_invdyn_refs as cref
import invdyn_refs
import wave_emu
from test_gpu_contact_parity import RTOL, _rel

pytestmark = pytest.mark.skipif(not os.path.exists(wave_emu.CLANG) or shutil.which("true") is None,
                                reason="needs the ROCm clang for the host build")

B = 2


def _run(world, st, a, frame, wrench, bodies, guesses):
    exe = wave_emu.build("contact_invdyn_emu")
    lines = invdyn_refs.desc_lines(world)
    f = wave_emu._fmt
    lines += [str(st.shape[0]), f(st), f(a), str(frame), f(wrench), str(len(bodies)), f(bodies, True),
              "0" if guesses is None else "1"]
    if guesses is not None:
        lines.append(f(guesses))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], input="\n".join(lines), capture_output=True, text=True, timeout=1800, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    out = {}
    for ln in r.stdout.splitlines():
        t = ln.split()
        out[t[0]] = np.array([float(x) for x in t[1:]])
    return out


@pytest.fixture(scope="module")
def rig():
    world = cref.rig_world()
    st, a = cref.rig_states(world, B, seed=11)
    nb = int(world.desc_arrays()["num_bodies"])
    wrench = 0.5 * np.random.default_rng(12).standard_normal((B, nb, 6))
    return world, st, a, wrench


@pytest.mark.parametrize("case", ["k1", "k2", "k3_guesses"])
def test_contact_inverse_dynamics_emulated(rig, case):
    world, st, a, wrench = rig
    n = world.getNumDofs()
    d = world.desc_arrays()
    nb = int(d["num_bodies"])
    assert n == 12 and nb == 9 and np.any(np.asarray(d["damping"]) != 0) and np.any(np.asarray(d["spring"]) != 0)
    skel = world.getSkeleton("rig")
    names = {"k1": ["l_foot"], "k2": ["l_foot", "r_foot"], "k3_guesses": ["l_foot", "r_foot", "arm"]}[case]
    from nimblephysics_amd.contact_inverse_dynamics import contact_body_indices
    bodies = contact_body_indices(world, [skel.getBodyNode(x) for x in names])
    k = len(bodies)
    guesses = 5.0 * np.random.default_rng(13).standard_normal((B, k, 6)) if case == "k3_guesses" else None
    out = _run(world, st, a, 1, wrench, bodies, guesses)
    tau, F, full = out["tau"].reshape(B, n), out["F"].reshape(B, k, 6), out["full"].reshape(B, n)
    gw = out["gw"].reshape(B, n, nb, 6)
    e = {}
    # tau_full of the emulation without the wrench's part against the oracle:
    # the wrench enters linearly through the same Jacobians
    Jall = -np.transpose(gw, (0, 2, 3, 1))  # [B, nb, 6, n]
    ref = invdyn_refs.Ref(world)
    ext = np.einsum("bkin,bki->bn", Jall, wrench)
    e["tau_full"] = _rel(full + ext, ref.tau_batch(st, a))
    rt, rF = np.zeros_like(tau), np.zeros_like(F)
    for b in range(B):
        J = Jall[b, bodies].reshape(6 * k, n)
        rt[b], rF[b], cond = cref.reference(full[b], J, 0, None if guesses is None else guesses[b])
        assert cond <= 1e8, cond
        e["closure"] = max(e.get("closure", 0.0), _rel((full[b] - tau[b])[6:], (J.T @ F[b].reshape(-1))[6:]))
    e["tau"] = _rel(tau, rt)
    e["F"] = _rel(F, rF)
    print(case, {key: f"{v:.2e}" for key, v in e.items()})
    assert np.all(tau[:, :6] == 0.0) and not np.any(np.signbit(tau[:, :6]))
    assert np.abs(tau[:, 6:]).min() > 1e-6 and np.abs(F).min() > 1e-9
    for key, v in e.items():
        assert v <= RTOL, (case, key, v)
