"""Inverse dynamics, the host side (no device): the ctypes prototypes of the
two entry points against the header, the DeviceWorld wrappers' shape / dtype /
frame validation, the rejection of a differentiable ``mass``, and the guard of
the bar itself -- the two CPU references the device tests lean on
(invdyn_refs.py: the oracle's analytic step Jacobian turned into the Jacobian
of ID, and Richardson-extrapolated central differences of the oracle's tau)
must agree with each other to RTOL / 10 on every model the device tests use.

Results before this feature: FEATURE MISSING -- _native.ID_PROTOTYPES,
DeviceWorld.inverse_dynamics, nimblephysics_amd.inverse_dynamics and the
header's declarations do not exist, so the first three tests fail on the
parent commit (the reference-agreement test exercises only the oracle).

Observed agreement of the two references under _rel (bar RTOL / 10 = 1e-7):
g^T J (floor 1e-5) cartpole 9.2e-13, KR5 1.3e-8, Atlas 9.2e-9, ball 7.5e-9,
compound 1.2e-8; full Jacobian (floor 1e-4) at most 7.8e-9 (compound).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import invdyn_refs
import models
import nimblephysics_amd as nimble
from nimblephysics_amd import _native
from test_gpu_contact_parity import RTOL, _rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ctypes_prototypes_match_the_header():
    text = open(os.path.join(ROOT, "include", "nimble_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = {m.group(1): [a.strip() for a in m.group(2).split(",")]
            for m in re.finditer(r"\bint\s+(nimble_inverse_dynamics\w*)\s*\(([^)]*)\)\s*;", text)}
    names = ["nimble_inverse_dynamics", "nimble_inverse_dynamics_backward"]
    assert sorted(decl) == sorted(names) == sorted(_native.ID_PROTOTYPES)
    for name in names:
        args, proto = decl[name], _native.ID_PROTOTYPES[name]
        assert len(args) == len(proto), (name, len(args), len(proto))
        for a, t in zip(args, proto):
            # int32_t batch / wrench_frame by value, everything else a pointer
            assert (t is C.c_int32) == a.startswith("int32_t"), (name, a, t)
            assert (t is C.c_void_p) == ("*" in a or a.startswith("nimble_world_t")), (name, a, t)
        tail = [a.split()[-1].lstrip("*") for a in args]
        assert tail[:7] == ["world", "batch", "state", "ddq", "body_inertia", "body_wrench", "wrench_frame"], tail
        assert tail[-1] == "stream"
    assert [a.split()[-1].lstrip("*") for a in decl[names[0]]][7:10] == ["tau", "mass_matrix", "bias"]
    assert [a.split()[-1].lstrip("*") for a in decl[names[1]]][7:11] == ["grad_tau", "grad_state", "grad_ddq",
                                                                          "grad_wrench"]
    # each cites the reference line it replaces
    full = open(os.path.join(ROOT, "include", "nimble_amd.h")).read()
    for cite in ("Skeleton.cpp:9433", "World.cpp:1974", "World.cpp:1943", "Skeleton.cpp:1884"):
        assert cite in full, cite


def test_shape_dtype_and_frame_validation_without_a_device():
    dev = object.__new__(_native.DeviceWorld)
    dev.nb, dev.n, dev.device_index = 3, 4, 0
    dev.h = None  # (nothing to release)
    B = 2
    z = lambda *s: torch.zeros(s, dtype=torch.float64)  # noqa: E731
    st, a, tau = z(B, 8), z(B, 4), z(B, 4)
    # well-formed CPU tensors pass every shape check and stop at the device check
    with pytest.raises(RuntimeError, match="ROCm device only"):
        dev.inverse_dynamics(st, a, tau, 0, mass_matrix=z(B, 4, 4), bias=z(B, 4), body_inertia=z(B, 3, 10),
                             body_wrench=z(B, 3, 6), wrench_frame="body")
    with pytest.raises(RuntimeError, match="ROCm device only"):
        dev.inverse_dynamics_backward(st, a, z(B, 4), z(B, 8), z(B, 4), 0, body_wrench=z(B, 3, 6),
                                      grad_wrench=z(B, 3, 6))
    bad = [
        (ValueError, lambda: dev.inverse_dynamics(z(B, 7), a, tau, 0)),
        (ValueError, lambda: dev.inverse_dynamics(z(8), z(4), z(4), 0)),
        (ValueError, lambda: dev.inverse_dynamics(st, z(B, 5), tau, 0)),
        (ValueError, lambda: dev.inverse_dynamics(st, a, z(B + 1, 4), 0)),
        (ValueError, lambda: dev.inverse_dynamics(st, a, tau, 0, mass_matrix=z(B, 4, 3))),
        (ValueError, lambda: dev.inverse_dynamics(st, a, tau, 0, bias=z(B, 8))),
        (TypeError, lambda: dev.inverse_dynamics(st.float(), a, tau, 0)),
        (TypeError, lambda: dev.inverse_dynamics(st, a, tau, 0, bias=z(B, 4).float())),
        (ValueError, lambda: dev.inverse_dynamics(st, a.t().contiguous().t(), tau, 0)),
        (ValueError, lambda: dev.inverse_dynamics(st, a, tau, 0, body_inertia=z(B, 3, 9))),
        (ValueError, lambda: dev.inverse_dynamics(st, a, tau, 0, body_wrench=z(B, 2, 6))),
        (TypeError, lambda: dev.inverse_dynamics(st, a, tau, 0, body_wrench=z(B, 3, 6).float())),
        (ValueError, lambda: dev.inverse_dynamics(st, a, tau, 0, body_wrench=z(B, 3, 6), wrench_frame="local")),
        (ValueError, lambda: dev.inverse_dynamics(st, a, tau, 0, wrench_frame=2)),
        (ValueError, lambda: dev.inverse_dynamics_backward(st, a, z(B, 5), z(B, 8), z(B, 4), 0)),
        (ValueError, lambda: dev.inverse_dynamics_backward(st, a, z(B, 4), z(B, 4), z(B, 4), 0)),
        (ValueError, lambda: dev.inverse_dynamics_backward(st, a, z(B, 4), z(B, 8), z(B, 8), 0)),
        (ValueError, lambda: dev.inverse_dynamics_backward(st, a, z(B, 4), z(B, 8), z(B, 4), 0,
                                                           body_wrench=z(B, 3, 6), grad_wrench=z(B, 3, 5))),
        (ValueError, lambda: dev.inverse_dynamics_backward(st, a, z(B, 4), z(B, 8), z(B, 4), 0,
                                                           grad_wrench=z(B, 3, 6))),
    ]
    for exc, call in bad:
        with pytest.raises(exc):
            call()


def test_layer_argument_checks_without_a_device():
    w = models.cartpole_world()
    w.tuneMass(w.getSkeleton(0).getBodyNode(1), "INERTIA_MASS")
    n = w.getNumDofs()
    st, a = torch.zeros(2 * n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    m = torch.ones(w.getMassDims(), dtype=torch.float64, requires_grad=True)
    with pytest.raises(ValueError, match="not differentiable"):
        nimble.inverse_dynamics(w, st, a, mass=m)
    with pytest.raises(ValueError, match="not differentiable"):
        nimble.inverse_dynamics(w, st.reshape(1, -1), a.reshape(1, -1), mass=m.reshape(1, -1))
    with pytest.raises(ValueError):
        nimble.inverse_dynamics(w, st, a, wrench_frame="sideways")
    with pytest.raises(ValueError, match="body_wrench must be"):
        nimble.inverse_dynamics(w, st, a, body_wrench=torch.zeros((1, w.getNumBodyNodes(), 6), dtype=torch.float64))
    assert nimble.InverseDynamicsLayer.apply and nimble.mass_matrix and nimble.coriolis_and_gravity
    assert callable(w.getMassMatrix) and callable(w.getCoriolisAndGravityForces)
    with pytest.raises(ValueError):
        nimble.mass_matrix(w, torch.zeros(n + 1, dtype=torch.float64))


def _case(name):
    if name == "cartpole":
        w = invdyn_refs.damped_cartpole()
        st, _ = models.random_states(w, 1, seed=3, q_scale=0.5, v_scale=1.0)
    elif name == "kr5":
        w = models.kr5_world()
        st, _ = models.random_states(w, 1, seed=3, q_scale=0.5, v_scale=1.0)
    elif name == "atlas":
        w = models.atlas_world(False)
        st, _ = models.random_states(w, 1, seed=3, q_scale=0.2, v_scale=0.3)
    elif name == "ball":
        w = models.ball_world(ground=False)
        st, _ = models.ball_states(1, seed=21, contact=False)
    else:
        w = models.compound_world(ground=False)
        st, _ = models.compound_states(1, seed=21, contact=False)
    return w, st[0]


@pytest.mark.parametrize("name", ["cartpole", "kr5", "atlas", "ball", "compound"])
def test_the_two_references_agree(name):
    """Guards the bar: the analytic reference and the Richardson reference,
    independent of each other, agree ten times inside it."""
    w, st = _case(name)
    n = w.getNumDofs()
    ref = invdyn_refs.Ref(w)
    q, v = st[:n], st[n:]
    a = invdyn_refs.accelerations(n, seed=5)
    # the oracle round trip: forward dynamics of tau_ref gives a back
    back = ref.o.forward_dynamics(q, v, ref.tau(q, v, a))
    assert np.abs(back - a).max() <= 1e-11 * max(1.0, np.abs(a).max())
    JA = np.hstack(ref.analytic(q, v, a))
    JR = np.hstack(ref.richardson(q, v, a))
    full = _rel(JA, JR, 1e-4)
    rng = np.random.default_rng(9)
    vjp = max(_rel(g @ JA, g @ JR, 1e-5) for g in rng.standard_normal((2, n)))
    print(name, f"g^T J {vjp:.2e}  full Jacobian {full:.2e}")
    assert vjp <= RTOL / 10 and full <= RTOL / 10, (name, vjp, full)
