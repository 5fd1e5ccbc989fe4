"""External body wrenches, the host side (no device): the world-order to
device-order scatter, argument validation, the reference-shaped BodyNode
setters and the ctypes prototypes of the `_ext` entry points.

Results before this feature: FEATURE MISSING -- World._scatter_wrench, the
setters and _native.EXT_PROTOTYPES do not exist, so every test here fails on
the parent commit.
"""
import os
import re

import numpy as np
import pytest
import torch

import models
from nimblephysics_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scatter_to_device_order_compound_rig():
    """The compound rig's device model holds the massless frames of its
    joint chains: they get zero rows, and the wrench of world body i lands on
    the device body that carries that BodyNode."""
    w = models.compound_world()
    model = w._model_bodies()
    bodies = w._world_bodies()
    nb, nbw = len(model), len(bodies)
    assert nbw == w.getNumBodyNodes() == 4 and nb > nbw
    W = torch.arange(2 * nbw * 6, dtype=torch.float64).reshape(2, nbw, 6) + 1.0
    out = w._scatter_wrench(W)
    assert tuple(out.shape) == (2, nb, 6) and out.dtype == torch.float64
    seen = 0
    for k, e in enumerate(model):
        if e[2] is None:
            assert not out[:, k].any()          # chain frame
        else:
            i = next(j for j, b in enumerate(bodies) if b is e[2])
            assert torch.equal(out[:, k], W[:, i])
            seen += 1
    assert seen == nbw
    # device bodies are the description's: same count, masses of the carried BodyNodes
    d = w.desc_arrays()
    assert int(d["num_bodies"]) == nb
    rows = w._wrench_device_rows()
    assert [d["mass"][k] for k in rows] == [b.getMass() for b in bodies]
    # and back
    assert torch.equal(w._gather_wrench(out), W)
    # a model without chains: the identity
    c = models.cartpole_world()
    Wc = torch.ones((3, c.getNumBodyNodes(), 6), dtype=torch.float64)
    assert torch.equal(c._scatter_wrench(Wc), Wc)


def test_shape_and_frame_validation():
    w = models.compound_world()
    nbw = w.getNumBodyNodes()
    with pytest.raises(ValueError):
        w._scatter_wrench(torch.zeros((2, nbw + 1, 6), dtype=torch.float64))
    with pytest.raises(ValueError):
        w._scatter_wrench(torch.zeros((2, nbw, 5), dtype=torch.float64))
    with pytest.raises(ValueError):
        w._scatter_wrench(torch.zeros((nbw, 6), dtype=torch.float64))
    assert _native.wrench_frame_flag("world") == 0 and _native.wrench_frame_flag("body") == 1
    assert _native.wrench_frame_flag(1) == 1
    for bad in ("local", "WORLD", 2, None, True):
        with pytest.raises(ValueError):
            _native.wrench_frame_flag(bad)
    # the DeviceWorld wrapper's own checks need no device either
    dev = object.__new__(_native.DeviceWorld)
    dev.nb, dev.n = 7, 8
    ok = torch.zeros((2, 7, 6), dtype=torch.float64)
    assert dev._wrench(2, ok, "body") == 1 and dev._wrench(2, None, "world") == 0
    with pytest.raises(ValueError):
        dev._wrench(2, torch.zeros((2, 6, 6), dtype=torch.float64), "world")
    with pytest.raises(TypeError):
        dev._wrench(2, ok.float(), "world")
    with pytest.raises(ValueError):
        dev._wrench(2, ok.transpose(1, 2).contiguous().transpose(1, 2), "world")
    with pytest.raises(ValueError):
        dev._wrench(2, ok, "world", grad_wrench=torch.zeros((2, 7, 5), dtype=torch.float64))
    with pytest.raises(ValueError):
        dev._wrench(2, None, "world", grad_wrench=ok)
    with pytest.raises(ValueError):
        dev._wrench(2, ok, "sideways")
    dev.h = None  # (nothing to release)


def test_body_node_setters():
    """BodyNode.cpp:1532-1612 for the body-frame variants; the others raise
    NotImplementedError naming wrench_frame="world"."""
    w = models.compound_world()
    skel = w.getSkeleton(0)
    b = skel.getBodyNode(1)
    version = w._version
    assert np.array_equal(b.getExternalForceLocal(), np.zeros(6)) and w._stored_wrench() is None
    b.setExtWrench([1, 2, 3, 4, 5, 6])
    assert np.array_equal(b.getExternalForceLocal(), [1, 2, 3, 4, 5, 6])
    b.addExtTorque([1, 1, 1], True)
    assert np.array_equal(b.getExternalForceLocal(), [2, 3, 4, 4, 5, 6])
    b.setExtTorque([0, 0, 1], True)
    assert np.array_equal(b.getExternalForceLocal(), [0, 0, 1, 4, 5, 6])
    f, o = np.array([0.0, 2.0, 0.0]), np.array([0.5, 0.0, 0.0])
    b.setExtForce(f, o, True, True)   # replaces mFext: [o x f; f]
    assert np.array_equal(b.getExternalForceLocal(), [0, 0, 1.0, 0, 2.0, 0])
    b.addExtForce(f, o, True, True)
    assert np.array_equal(b.getExternalForceLocal(), [0, 0, 2.0, 0, 4.0, 0])
    stored = w._stored_wrench()
    assert stored.shape == (w.getNumBodyNodes(), 6) and np.array_equal(stored[1], [0, 0, 2.0, 0, 4.0, 0])
    assert not stored[[0, 2, 3]].any()
    assert w._version == version       # an input of the step, not a model change
    for call in (lambda: b.addExtForce(f), lambda: b.addExtForce(f, o, False, True),
                 lambda: b.addExtForce(f, o, True, False), lambda: b.setExtForce(f, o, False, False),
                 lambda: b.addExtTorque(f), lambda: b.setExtTorque(f, False)):
        with pytest.raises(NotImplementedError, match='wrench_frame="world"'):
            call()
    with pytest.raises(ValueError):
        b.setExtWrench([1, 2, 3])
    skel.getBodyNode(0).setExtWrench(np.ones(6))
    skel.clearExternalForces()
    assert w._stored_wrench() is None
    b.setExtWrench(np.ones(6))
    b.clearExternalForces()
    assert not b.getExternalForceLocal().any()
    b.setExtWrench(np.ones(6))
    w.clearExternalForces()
    assert w._stored_wrench() is None


def _header_arg_counts():
    text = open(os.path.join(ROOT, "include", "nimble_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(nimble_\w+_ext)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = [a.strip() for a in m.group(2).split(",")]
    return out


def test_ctypes_prototypes_match_the_header():
    decl = _header_arg_counts()
    names = ["nimble_forward_ext", "nimble_backward_ext", "nimble_backward_masses_ext", "nimble_backward_inertia_ext",
             "nimble_jacobians_ext", "nimble_constraint_force_jacobians_ext"]
    assert sorted(decl) == sorted(names) == sorted(_native.EXT_PROTOTYPES)
    import ctypes as C
    for name in names:
        args, proto = decl[name], _native.EXT_PROTOTYPES[name]
        assert len(args) == len(proto), (name, len(args), len(proto))
        for a, t in zip(args, proto):
            # int32_t batch / wrench_frame by value, everything else a pointer
            assert (t is C.c_int32) == a.startswith("int32_t"), (name, a, t)
            assert (t is C.c_void_p) == ("*" in a or a.startswith("nimble_world_t")), (name, a, t)
        frame = [i for i, a in enumerate(args) if a.endswith("wrench_frame")]
        wrench = [i for i, a in enumerate(args) if a.endswith("body_wrench")]
        inertia = [i for i, a in enumerate(args) if a.endswith("body_inertia")]
        assert len(frame) == 1 and wrench == [frame[0] - 1] and inertia == [frame[0] - 2], (name, args)
        assert args[-1].endswith("stream")
