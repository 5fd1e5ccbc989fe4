"""The inverse-dynamics kernels for the inertial parameters on the CPU:
nimble_inverse_dynamics_backward_inertia_kernel and
nimble_inverse_dynamics_inertia_jacobian_kernel compiled for the host with
AddressSanitizer against the emulated wavefront (tests/cpp/wave_emu,
invdyn_inertia_emu.cpp, a stand-alone executable; nothing is loaded into
Python) and run through the emulated C ABI on the damped cartpole and on the
compound rig without ground (8 device bodies, 5 of them massless chain
frames), B = 2, world b on parameter set b of per_world_params.  The Jacobian
is checked against the oracle's central-difference columns
(invdyn_inertia_refs.py: exact up to rounding, tau being a polynomial in the
parameters), grad_inertia against g^T J of the same reference and against the
Jacobian kernel's own output; elements off the root path are exactly 0.0, the
outputs start as NaN and every element is written, grad_state and grad_ddq
are the bits of nimble_inverse_dynamics_backward, and any out-of-bounds access
aborts the run.  No GPU needed.

Results before this feature: FEATURE MISSING -- the driver and the entry
points it calls do not exist, so every test here fails on the parent commit.

Observed maxima under _rel (floor 1e-5), bar RTOL = 1e-6, cartpole /
compound: reference columns at the steps vs half steps 1.7e-14 / 9.6e-10,
Richardson direction vs J d 1.3e-15 / 2.8e-15 (bar 1e-7); Jacobian 3.4e-15 /
1.0e-9, grad_inertia vs g^T J_ref 3.2e-15 / 9.9e-10, vs the Jacobian kernel
3.4e-16 / 1.6e-14.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import invdyn_inertia_refs as refs
import invdyn_refs
import wave_emu
from test_gpu_contact_parity import RTOL, _rel

pytestmark = pytest.mark.skipif(not os.path.exists(wave_emu.CLANG) or shutil.which("true") is None,
                                reason="needs the ROCm clang for the host build")


def _run(world, st, a, g, P):
    exe = wave_emu.build("invdyn_inertia_emu")
    lines = invdyn_refs.desc_lines(world)
    f = wave_emu._fmt
    lines += [str(st.shape[0]), f(st), f(a), f(g), f(P)]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], input="\n".join(lines), capture_output=True, text=True, timeout=1800, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    out = {}
    for ln in r.stdout.splitlines():
        t = ln.split()
        out[t[0]] = np.array([float(x) for x in t[1:]])
    return out


@pytest.mark.parametrize("name", ["cartpole", "compound"])
def test_inertia_kernels_emulated(name):
    B = 2
    c = refs.case(name, B)
    world, st, a, P = c["world"], c["st"], c["a"], c["P"]
    n, nb = world.getNumDofs(), P.shape[1]
    assert c["half"] <= RTOL / 10 and c["rich"] <= RTOL / 10, (c["half"], c["rich"])
    g = np.random.default_rng(6).standard_normal((B, n))
    out = _run(world, st, a, g, P)
    jac, gi = out["jac"].reshape(B, n, nb, 10), out["gi"].reshape(B, nb, 10)
    assert np.isfinite(jac).all() and np.isfinite(gi).all()
    d = world.desc_arrays()
    parent, dof0 = np.asarray(d["parent"]), np.asarray(d["dof_offset"])
    # (dof_offset is non-decreasing over the device bodies)
    dof_body = np.repeat(np.arange(nb), np.diff(np.append(dof0, n)))
    e = {"half": c["half"], "rich": c["rich"]}
    for b in range(B):
        for body in range(nb):
            path, k = set(), body
            while k >= 0:
                path.add(k)
                k = parent[k]
            off = [j for j in range(n) if dof_body[j] not in path]
            assert (jac[b][off, body, :] == 0.0).all() and not np.signbit(jac[b][off, body, :]).any()
        sel = c["bodies"][b]
        e["jacobian"] = max(e.get("jacobian", 0.0), _rel(jac[b][:, sel], c["J"][b][:, sel]))
        e["grad_inertia"] = max(e.get("grad_inertia", 0.0),
                                _rel(gi[b][sel], np.einsum("j,jbp->bp", g[b], c["J"][b])[sel]))
    e["grad_inertia vs jacobian"] = _rel(gi, np.einsum("bj,bjkp->bkp", g, jac))
    print(name, {k: f"{v:.2e}" for k, v in e.items()})
    for k, v in e.items():
        assert v <= RTOL, (name, k, v)
    # the chain frames' rows are written and, their dofs moving, not all zero
    if name == "compound":
        chain = [k for k in range(nb) if k not in refs.massive(world)]
        assert len(chain) == 5 and np.abs(gi[:, chain]).max() > 0
    assert np.array_equal(out["gs"], out["gs0"]) and np.array_equal(out["ga"], out["ga0"])
