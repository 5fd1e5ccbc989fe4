"""Inverse dynamics in the inertial parameters, the host side (no device): the
ctypes prototypes of the two entry points against the header and the built
library, World.getBodyInertiaParameters (values and autograd gradient for
every entry kind, the later-entry-wins case included), every ValueError of the
new keyword and function, and the DeviceWorld wrappers' shape checks, which
well-formed CPU tensors pass up to the device check.

Results before this feature: FEATURE MISSING -- _native.ID_INERTIA_PROTOTYPES,
the header's declarations, World.getBodyInertiaParameters, the body_inertia
keyword and nimblephysics_amd.inverse_dynamics_inertia_jacobian do not exist,
so every test here fails on the parent commit.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import models
import nimblephysics_amd as nimble
from nimblephysics_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ctypes_prototypes_match_the_header_and_the_library():
    full = open(os.path.join(ROOT, "include", "nimble_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    decl = {m.group(1): [a.strip() for a in m.group(2).split(",")]
            for m in re.finditer(r"\bint\s+(nimble_invdyn\w*)\s*\(([^)]*)\)\s*;", text)}
    names = ["nimble_invdyn_backward_inertia", "nimble_invdyn_inertia_jacobian"]
    assert sorted(decl) == sorted(names) == sorted(_native.ID_INERTIA_PROTOTYPES)
    for name in names:
        args, proto = decl[name], _native.ID_INERTIA_PROTOTYPES[name]
        assert len(args) == len(proto), (name, len(args), len(proto))
        for a, t in zip(args, proto):
            assert (t is C.c_int32) == a.startswith("int32_t"), (name, a, t)
            assert (t is C.c_void_p) == ("*" in a or a.startswith("nimble_world_t")), (name, a, t)
    tail = lambda name: [a.split()[-1].lstrip("*") for a in decl[name]]  # noqa: E731
    # the backward's arguments with grad_inertia ahead of the stream
    back = re.search(r"\bint\s+nimble_inverse_dynamics_backward\s*\(([^)]*)\)\s*;", text).group(1)
    back = [a.strip().split()[-1].lstrip("*") for a in back.split(",")]
    assert tail(names[0]) == back[:-1] + ["grad_inertia", "stream"]
    assert tail(names[1]) == ["world", "batch", "state", "ddq", "body_inertia", "jacobian", "stream"]
    # each cites the reference interface it stands for
    for cite in ("Skeleton.cpp:1884", ":1832", ":1779", "WithRespectToMass.cpp:35", "GROUP_MASSES", "GROUP_COMS",
                 "GROUP_INERTIAS"):
        assert cite in full, cite
    # and the built library has them, bound with these argtypes
    lib = _native.lib()
    for name in names:
        assert getattr(lib, name).argtypes == _native.ID_INERTIA_PROTOTYPES[name]
        assert getattr(lib, name).restype is C.c_int


def _tuned_world():
    """The cartpole with every entry kind tuned, and the pole's COM tuned
    twice: INERTIA_COM first, INERTIA_FULL later."""
    w = models.cartpole_world()
    bodies = w._world_bodies()
    w.tuneMass(bodies[0], "INERTIA_MASS")
    w.tuneMass(bodies[1], "INERTIA_COM")
    w.tuneMass(bodies[0], "INERTIA_COM_MU")
    w.tuneMass(bodies[0], "INERTIA_DIAGONAL")
    w.tuneMass(bodies[0], "INERTIA_OFF_DIAGONAL")
    w.tuneMass(bodies[1], "INERTIA_FULL")
    return w


def test_body_inertia_parameters_values():
    w = _tuned_world()
    rows = torch.as_tensor(w._wrench_device_rows())
    base = torch.as_tensor(w._body_inertia_base())[rows]
    P0 = w.getBodyInertiaParameters()
    assert P0.dtype == torch.float64 and tuple(P0.shape) == (w.getNumBodyNodes(), 10)
    assert torch.equal(P0, base)
    D = w.getMassDims()
    m2 = torch.as_tensor(np.random.default_rng(0).uniform(0.5, 1.5, (3, D)))
    want = w._batched_inertia(m2)[:, rows]
    P2 = w.getBodyInertiaParameters(m2)
    assert tuple(P2.shape) == (3, w.getNumBodyNodes(), 10) and torch.equal(P2, want)
    P1 = w.getBodyInertiaParameters(m2[1])
    assert tuple(P1.shape) == (w.getNumBodyNodes(), 10) and torch.equal(P1, want[1])
    for bad in (torch.zeros(D + 1), torch.zeros(2, D + 1), torch.zeros(1, 2, D)):
        with pytest.raises(ValueError):
            w.getBodyInertiaParameters(bad.double())
    # a compound-joint chain: its massless frames have no rows
    cw = models.compound_world(ground=False)
    assert len(cw._model_bodies()) == 8
    assert tuple(cw.getBodyInertiaParameters().shape) == (cw.getNumBodyNodes(), 10) == (3, 10)


def test_body_inertia_parameters_gradient_follows_the_selection_plan():
    w = _tuned_world()
    D, nbw = w.getMassDims(), w.getNumBodyNodes()
    only_masses, S = w._mass_selection()
    assert not only_masses and S.shape == (nbw * 10, D)
    # the later entry wins: a component's earlier columns get no gradient
    S = S.copy()
    for r in range(S.shape[0]):
        cols = np.nonzero(S[r])[0]
        S[r, cols[:-1]] = 0.0
    # (the pole's COM is tuned by INERTIA_COM and by INERTIA_FULL)
    assert (np.count_nonzero(w._mass_selection()[1], axis=1) > 1).any()
    G = np.random.default_rng(1).standard_normal((2, nbw, 10))
    for shape in ((D,), (2, D)):
        m = torch.as_tensor(np.random.default_rng(2).uniform(0.5, 1.5, shape)).requires_grad_()
        P = w.getBodyInertiaParameters(m)
        Gt = torch.as_tensor(G[0] if len(shape) == 1 else G)
        (P * Gt).sum().backward()
        want = (G[0].reshape(-1) @ S) if len(shape) == 1 else G.reshape(2, -1) @ S
        assert np.abs(m.grad.numpy() - want).max() <= 1e-15 * np.abs(want).max()
    # the beta factors of INERTIA_COM_MU are in S
    beta = w._world_bodies()[0].getBeta()
    col = 1 + 3  # INERTIA_MASS (1), INERTIA_COM (3), then INERTIA_COM_MU of the first body
    assert np.any(beta != 0) and np.array_equal(S[1:4, col], beta)


def test_layer_argument_checks_without_a_device():
    w = models.cartpole_world()
    w.tuneMass(w.getSkeleton(0).getBodyNode(1), "INERTIA_MASS")
    n, nbw = w.getNumDofs(), w.getNumBodyNodes()
    z = lambda *s: torch.zeros(s, dtype=torch.float64)  # noqa: E731
    st, a = z(2 * n), z(n)
    P = w.getBodyInertiaParameters()
    with pytest.raises(ValueError, match="not both"):
        nimble.inverse_dynamics(w, st, a, mass=torch.ones(1, dtype=torch.float64), body_inertia=P)
    # mass keeps its behaviour; the message names the route
    with pytest.raises(ValueError, match="not differentiable.*getBodyInertiaParameters"):
        nimble.inverse_dynamics(w, st, a, mass=torch.ones(1, dtype=torch.float64, requires_grad=True))
    bad1 = (z(nbw, 9), z(nbw + 1, 10), z(10), z(1, nbw, 10), z(1, 1, nbw, 10))
    bad2 = (z(nbw, 9), z(nbw + 1, 10), z(3, nbw, 10), z(2, nbw + 1, 10), z(2, nbw, 10, 1))
    for fn in (nimble.inverse_dynamics, nimble.inverse_dynamics_inertia_jacobian):
        for bad in bad1:
            with pytest.raises(ValueError, match="body_inertia"):
                fn(w, st, a, body_inertia=bad)
        for bad in bad2:
            with pytest.raises(ValueError, match="body_inertia"):
                fn(w, z(2, 2 * n), z(2, n), body_inertia=bad)
    with pytest.raises(ValueError):
        nimble.inverse_dynamics_inertia_jacobian(w, z(2 * n + 1), a)
    with pytest.raises(ValueError):
        nimble.inverse_dynamics_inertia_jacobian(w, st, z(1, n))
    assert "inverse_dynamics_inertia_jacobian" in nimble.__all__


def test_shape_checks_of_the_wrappers_without_a_device():
    dev = object.__new__(_native.DeviceWorld)
    dev.nb, dev.n, dev.device_index = 3, 4, 0
    dev.h = None  # (nothing to release)
    B = 2
    z = lambda *s: torch.zeros(s, dtype=torch.float64)  # noqa: E731
    st, a = z(B, 8), z(B, 4)
    # well-formed CPU tensors pass every shape check and stop at the device check
    with pytest.raises(RuntimeError, match="ROCm device only"):
        dev.inverse_dynamics_backward(st, a, z(B, 4), z(B, 8), z(B, 4), 0, body_inertia=z(B, 3, 10),
                                      body_wrench=z(B, 3, 6), grad_wrench=z(B, 3, 6), grad_inertia=z(B, 3, 10))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        dev.inverse_dynamics_inertia_jacobian(st, a, z(B, 4, 3, 10), 0, body_inertia=z(B, 3, 10))
    bad = [
        (ValueError, lambda: dev.inverse_dynamics_backward(st, a, z(B, 4), z(B, 8), z(B, 4), 0,
                                                           grad_inertia=z(B, 3, 9))),
        (ValueError, lambda: dev.inverse_dynamics_backward(st, a, z(B, 4), z(B, 8), z(B, 4), 0,
                                                           grad_inertia=z(B + 1, 3, 10))),
        (TypeError, lambda: dev.inverse_dynamics_backward(st, a, z(B, 4), z(B, 8), z(B, 4), 0,
                                                          grad_inertia=z(B, 3, 10).float())),
        (ValueError, lambda: dev.inverse_dynamics_backward(st, a, z(B, 4), z(B, 8), z(B, 4), 0,
                                                           grad_inertia=z(B, 10, 3).transpose(1, 2))),
        (ValueError, lambda: dev.inverse_dynamics_inertia_jacobian(st, a, None, 0)),
        (ValueError, lambda: dev.inverse_dynamics_inertia_jacobian(st, a, z(B, 3, 4, 10), 0)),
        (ValueError, lambda: dev.inverse_dynamics_inertia_jacobian(st, a, z(B, 4, 3, 9), 0)),
        (ValueError, lambda: dev.inverse_dynamics_inertia_jacobian(z(B, 7), a, z(B, 4, 3, 10), 0)),
        (ValueError, lambda: dev.inverse_dynamics_inertia_jacobian(st, z(B, 5), z(B, 4, 3, 10), 0)),
        (ValueError, lambda: dev.inverse_dynamics_inertia_jacobian(st, a, z(B, 4, 3, 10), 0,
                                                                   body_inertia=z(B, 4, 10))),
        (TypeError, lambda: dev.inverse_dynamics_inertia_jacobian(st, a, z(B, 4, 3, 10).float(), 0)),
    ]
    for exc, call in bad:
        with pytest.raises(exc):
            call()
