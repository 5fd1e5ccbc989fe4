"""Host side of the per-world body inertial parameters (no GPU):

* World._batched_inertia expands [B, getMassDims()] mass vectors to the
  kernels' [B, nb, 10] array exactly as setMasses would have written each row
  into the world's bodies, for every WrtMassBodyNodeEntryType (COM_MU with a
  beta off the axes) and for a compound-joint world, whose device bodies
  outnumber its BodyNodes -- with torch ops on the mass tensor's device and
  without touching the world;
* the DeviceWorld wrappers reject a body_inertia of the wrong shape, dtype or
  layout before any native call.
"""
import numpy as np
import pytest
import torch

import models
import per_world_params as PW
from nimblephysics_amd import _native


def _readback(world, row):
    """The [nb, 10] array of the world after setMasses(row), restored after."""
    m0 = world.getMasses()
    try:
        world.setMasses(row)
        return world._body_inertia_base()
    finally:
        world.setMasses(m0)


def _rows(world, B, seed):
    rng = np.random.default_rng(seed)
    m0 = world.getMasses()
    return m0[None, :] * (1.0 + 0.2 * rng.uniform(-1, 1, (B, len(m0)))) + 0.01 * rng.standard_normal((B, len(m0)))


def _check(world, B=5, seed=0):
    mass = _rows(world, B, seed)
    version, m0 = world._version, world.getMasses().copy()
    base0 = world._body_inertia_base().copy()
    got = world._batched_inertia(torch.tensor(mass))
    assert world._version == version and np.array_equal(world.getMasses(), m0)
    assert np.array_equal(world._body_inertia_base(), base0)
    nb = len(world._model_bodies())
    assert tuple(got.shape) == (B, nb, 10) and got.dtype == torch.float64 and got.is_contiguous()
    assert got.device.type == "cpu"
    for b in range(B):
        assert np.array_equal(got[b].numpy(), _readback(world, mass[b])), b
    return got.numpy()


def test_every_entry_type_atlas():
    w = models.atlas_world(True)
    bodies = [b for s in w.skeletons for b in s.bodies]
    bodies[27].setBeta([0.3, -1.0, 0.5])
    bodies[27].setLocalCOM(bodies[27].getBeta() * 0.04)
    w.tuneMass(bodies[0], "INERTIA_MASS")
    w.tuneMass(bodies[3], "INERTIA_COM")
    w.tuneMass(bodies[27], "INERTIA_COM_MU")
    w.tuneMass(bodies[27], "INERTIA_DIAGONAL")
    w.tuneMass(bodies[9], "INERTIA_OFF_DIAGONAL")
    w.tuneMass(bodies[5], "INERTIA_FULL")
    assert w.getMassDims() == 1 + 3 + 1 + 3 + 3 + 10
    got = _check(w)
    base = w._body_inertia_base()
    # bodies without a tuned entry keep the model's values in every world
    untouched = [i for i in range(len(base)) if i not in (0, 3, 27, 9, 5)]
    assert np.array_equal(got[:, untouched], np.broadcast_to(base[untouched], got[:, untouched].shape))
    # and the rows differ from one another where they are tuned
    assert not np.array_equal(got[0, 27], got[1, 27])


def test_masses_only():
    w = models.atlas_world(True)
    bodies = [b for s in w.skeletons for b in s.bodies]
    w.tuneMass(bodies[27], "INERTIA_MASS")
    w.tuneMass(bodies[0], "INERTIA_MASS")
    assert w._mass_selection()[0]
    _check(w, seed=1)


def test_compound_world_device_bodies():
    """Massless chain frames precede the BodyNodes of compound joints: the
    rows are in device-model order and the frames stay zero."""
    w = models.compound_world()
    bodies = [b for s in w.skeletons for b in s.bodies]
    nb = len(w._model_bodies())
    assert nb > len(bodies)
    w.tuneMass(bodies[1], "INERTIA_FULL")
    w.tuneMass(bodies[2], "INERTIA_MASS")
    w.tuneMass(bodies[0], "INERTIA_COM_MU")
    bodies[0].setBeta([0.0, 0.5, 2.0])
    got = _check(w, seed=2)
    frames = [i for i, e in enumerate(w._model_bodies()) if e[2] is None]
    assert frames and not got[:, frames].any()
    assert got.shape[1] == int(w.desc_arrays()["num_bodies"])


def test_later_entry_wins_like_setmasses():
    """Two entries on one component (FULL after MASS): the later value."""
    w = models.cartpole_world()
    bodies = [b for s in w.skeletons for b in s.bodies]
    w.tuneMass(bodies[1], "INERTIA_MASS")
    w.tuneMass(bodies[1], "INERTIA_FULL")
    _check(w, seed=3)


def test_param_sets_are_positive_definite():
    for make in (models.cartpole_world, lambda: models.atlas_world(True), models.half_cheetah_world,
                 models.compound_world):
        w = make()
        sets = PW.param_sets(w)
        assert np.array_equal(sets[0], PW.base_params(w))
        for P in sets:
            assert PW.positive_definite(P)
        # (COM shifts of at most 2 cm, up to the rounding of the sum)
        assert np.abs(sets[1][:, 1:4] - sets[0][:, 1:4]).max() <= 0.02 + 1e-15
        assert np.abs(sets[2][:, 1:4] - sets[0][:, 1:4]).max() <= 0.02 + 1e-15


def test_wrong_shapes_raise():
    w = models.cartpole_world()
    bodies = [b for s in w.skeletons for b in s.bodies]
    w.tuneMass(bodies[1], "INERTIA_MASS")
    with pytest.raises(ValueError):
        w._batched_inertia(torch.zeros(4, 2, dtype=torch.float64))
    with pytest.raises(ValueError):
        w._batched_inertia(torch.zeros(1, dtype=torch.float64))


def test_device_wrappers_check_body_inertia_first(monkeypatch):
    """Shape / dtype / layout errors of body_inertia come before any native
    call (and before anything needs a device)."""
    def no_native():
        raise AssertionError("native library reached")
    monkeypatch.setattr(_native, "lib", no_native)
    dev = object.__new__(_native.DeviceWorld)
    dev.h, dev.device_index, dev.n, dev.nb = None, 0, 2, 3
    dev.snapshot_doubles, dev.cache_doubles, dev.num_pairs = 8, 127, 0
    B = 4
    st, f = torch.zeros(B, 4, dtype=torch.float64), torch.zeros(B, 2, dtype=torch.float64)
    snap, cache = torch.zeros(B, 8, dtype=torch.float64), torch.zeros(B, 127, dtype=torch.float64)
    g, gs, gf = torch.zeros_like(st), torch.zeros_like(st), torch.zeros_like(f)
    gm, gi = torch.zeros(B, 3, dtype=torch.float64), torch.zeros(B, 3, 10, dtype=torch.float64)
    calls = {
        "forward": lambda bi: dev.forward(st, f, cache, torch.zeros_like(st), snap, 0, body_inertia=bi),
        "backward": lambda bi: dev.backward(st, f, snap, g, gs, gf, 0, body_inertia=bi),
        "backward_masses": lambda bi: dev.backward_masses(st, f, snap, g, gs, gf, gm, 0, body_inertia=bi),
        "backward_inertia": lambda bi: dev.backward_inertia(st, f, snap, g, gs, gf, gi, 0, body_inertia=bi),
        "jacobians": lambda bi: dev.jacobians(st, f, snap, 0, body_inertia=bi),
        "constraint_force_jacobians": lambda bi: dev.constraint_force_jacobians(st, f, snap, 0, body_inertia=bi),
    }
    bad_shapes = [torch.zeros(B, 3, 9, dtype=torch.float64), torch.zeros(B + 1, 3, 10, dtype=torch.float64),
                  torch.zeros(B, 4, 10, dtype=torch.float64), torch.zeros(B, 30, dtype=torch.float64)]
    for name, call in calls.items():
        for t in bad_shapes:
            with pytest.raises(ValueError, match="body_inertia shape"):
                call(t)
        with pytest.raises(TypeError, match="float64"):
            call(torch.zeros(B, 3, 10, dtype=torch.float32))
        with pytest.raises(ValueError, match="contiguous"):
            call(torch.zeros(B, 10, 3, dtype=torch.float64).transpose(1, 2))
        # a well-formed array on the CPU is refused as every CPU buffer is
        with pytest.raises(RuntimeError, match="ROCm device only"):
            call(torch.zeros(B, 3, 10, dtype=torch.float64))
