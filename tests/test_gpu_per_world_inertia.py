"""Per-world body inertial parameters (body_inertia [B, nb, 10], the `_pw`
entry points) on the GPU.

The per-world kernels are the shared-model kernels with the three reads of a
body's mass, COM and moment redirected to the world's own row, arithmetic and
operation order unchanged.  So a per-world run must reproduce, world by world
and bit for bit, what the shared-model path gives for a device model built
with that world's parameters (tests 1-4; the shared-model path itself is
pinned to the oracle by the rest of the suite), and where no LCP can take
another path it must match the oracle built per parameter set (test 5).  The
parameter sets are per_world_params.param_sets: world b gets set b % 3.

Results before this feature: FEATURE MISSING -- the `_pw` symbols do not
exist and a 2-D mass raises ValueError, so every test here fails on the
parent commit.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import models
import per_world_params as PW
from nimblephysics_amd import _native, neural, workloads
from nimblephysics_amd.timestep import mass_gradient, step_batch
from oracle import oracle as O
from test_gpu_contact_parity import SN_M, SN_STATUS
from test_gpu_mass import _get_param, _set_param

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("next state", "LCP cache", "snapshot header", "f_c", "dynamics cache", "grad state", "grad forces",
           "grad masses", "grad inertia", "state Jacobian", "force Jacobian", "dF_c / d state", "dF_c / d forces")


def _dyn_cache_doubles(n, nb):
    """csrc/pool_sizes.h dynCacheDoubles: Tw, Sw, V, packed M, dinv, rhs."""
    return 12 * nb + 6 * n + 6 * nb + n * (n + 1) // 2 + n + n


def _run(world, st, f, g, bi=None, cache=None):
    """Forward, the three backward modes and both Jacobian modes through the
    DeviceWorld wrappers, with explicit zeroed buffers; `bi`: [B, nb, 10]
    numpy array for the per-world entry points.  Returns OUTPUTS as device
    tensors (the snapshot without its stamp and workspace slots: header,
    clamping impulses and the dynamics cache at its tail)."""
    dev = world.native()
    d = torch.device("cuda:0")
    B = st.shape[0]
    ts, tf, tg = torch.tensor(st, device=d), torch.tensor(f, device=d), torch.tensor(g, device=d)
    tbi = None if bi is None else torch.tensor(bi, device=d)
    if cache is None:
        cache = torch.zeros((B, dev.cache_doubles), dtype=torch.float64, device=d)
        cache[:, 0] = -1
    else:
        cache = cache.clone()
    nxt = torch.empty_like(ts)
    snap = torch.zeros((B, dev.snapshot_doubles), dtype=torch.float64, device=d)
    stream = torch.cuda.current_stream().cuda_stream
    dev.forward(ts, tf, cache, nxt, snap, stream, body_inertia=tbi)
    gs, gf = torch.empty_like(ts), torch.empty_like(tf)
    dev.backward(ts, tf, snap, tg, gs, gf, stream, body_inertia=tbi)
    gs1, gf1 = torch.empty_like(ts), torch.empty_like(tf)
    gm = torch.empty((B, dev.nb), dtype=torch.float64, device=d)
    dev.backward_masses(ts, tf, snap, tg, gs1, gf1, gm, stream, body_inertia=tbi)
    gs2, gf2 = torch.empty_like(ts), torch.empty_like(tf)
    gi = torch.empty((B, dev.nb, 10), dtype=torch.float64, device=d)
    dev.backward_inertia(ts, tf, snap, tg, gs2, gf2, gi, stream, body_inertia=tbi)
    J, F = dev.jacobians(ts, tf, snap, stream, body_inertia=tbi)
    Js, Jf = dev.constraint_force_jacobians(ts, tf, snap, stream, body_inertia=tbi)
    torch.cuda.synchronize()
    # the mass / inertia modes leave the state and force gradients as they are
    assert torch.equal(gs, gs1) and torch.equal(gs, gs2) and torch.equal(gf, gf1) and torch.equal(gf, gf2)
    if dev.num_pairs > 0:
        fc = snap[:, _native.SN_FC:_native.SN_FC + _native.MAX_LCP].clone()
        header = snap[:, :SN_STATUS + 1].clone()
    else:
        fc, header = snap[:, :0].clone(), snap[:, :8].clone()
    dyn = snap[:, dev.snapshot_doubles - _dyn_cache_doubles(dev.n, dev.nb):].clone()
    return (nxt, cache, header, fc, dyn, gs, gf, gm, gi, J, F, Js, Jf)


def _assert_rows_equal(name, got, ref, rows):
    for label, x, y in zip(OUTPUTS, got, ref):
        x, y = x[rows], y[rows]
        ne = (x != y) & ~(torch.isnan(x) & torch.isnan(y))  # (NaN where the other has NaN: the same)
        if bool(ne.any()):
            bad = torch.nonzero(ne.reshape(x.shape[0], -1).any(dim=1)).flatten().tolist()
            diff = float((x - y)[ne].abs().max())
            raise AssertionError(f"{name}: {label} differs in rows {[rows[i] for i in bad]} (max |diff| {diff:.3e})")


def _cartpole():
    w = models.cartpole_world()
    return w, models.random_states(w, 4, seed=2)


def _atlas_air():
    w = models.atlas_world(False)
    return w, models.random_states(w, 4, seed=3, q_scale=0.2, v_scale=0.3)


def _atlas_contact():
    w = models.atlas_world(True)
    return w, models.random_states(w, 8, seed=3, q_scale=0.01, v_scale=0.02)


def _half_cheetah():
    w = models.half_cheetah_world()
    return w, models.half_cheetah_states(w, 16, seed=4)


def _compound():
    w = models.compound_world()
    return w, models.compound_states(4, seed=1)


# STL-mesh Atlas, the sampler of tests/test_gpu_mesh.py: with seed 28 the
# oracle's LCP row counts of the first three worlds are 30, 39 and 69 (picked
# on the CPU), so three is the smallest batch with a world over 64 rows, that
# world (parameter set 2) takes nimble_backward_wide_kernel, and every
# parameter set is present.
MESH_SEED, MESH_B, MESH_WIDE_WORLD = 28, 3, 2


def _atlas_mesh():
    w = workloads.atlas_mesh_world(True)
    return w, workloads.random_states(w, MESH_B, seed=MESH_SEED, q_scale=0.02, v_scale=0.05)


MODELS = {"cartpole": _cartpole, "atlas_air": _atlas_air, "atlas_contact": _atlas_contact,
          "half_cheetah": _half_cheetah, "compound": _compound}


@functools.lru_cache(maxsize=None)
def _results(name, mesh=False):
    """Every run of one model, made once and shared by the tests: the shared
    path on a device model built per parameter set (world parameters written
    through the BodyNode setters), and the per-world path on the unchanged
    model with the model's own values and with the three sets."""
    world, (st, f) = (_atlas_mesh if mesh else MODELS[name])()
    world.setStatusPolicy("record")
    B = st.shape[0]
    g = np.random.default_rng(11).standard_normal(st.shape)
    sets = PW.param_sets(world)
    assert all(PW.positive_definite(P) for P in sets)
    shared = {}
    for k in (1, 2, 0):  # (set 0 last: the world is the model again)
        PW.set_world_params(world, sets[k])
        shared[k] = _run(world, st, f, g)
    assert np.array_equal(PW.base_params(world), sets[0])
    nb = world.native().nb
    assert sets[0].shape == (nb, 10)
    own = _run(world, st, f, g, bi=np.broadcast_to(sets[0], (B, nb, 10)).copy())
    per = _run(world, st, f, g, bi=PW.batch_params(world, B))
    return world, st, f, g, shared, own, per


@pytest.mark.parametrize("name", sorted(MODELS))
def test_same_parameters_same_bits(name):
    """Test 1: body_inertia filled with the model's own values gives the bits
    of the entry points without it, in every world and every output."""
    world, st, f, g, shared, own, per = _results(name)
    _assert_rows_equal(name, own, shared[0], list(range(st.shape[0])))
    dev = world.native()
    if name == "compound":
        assert dev.nb > sum(len(s.bodies) for s in world.skeletons)  # (massless chain frames)


def test_null_pointer_is_the_shared_path():
    """NULL / None once: nimble_forward_pw and nimble_backward_inertia_pw with
    a null body_inertia are the existing entry points."""
    world, st, f, g, shared, own, per = _results("atlas_contact")
    dev = world.native()
    d = torch.device("cuda:0")
    B = st.shape[0]
    ts, tf, tg = torch.tensor(st, device=d), torch.tensor(f, device=d), torch.tensor(g, device=d)
    cache = torch.zeros((B, dev.cache_doubles), dtype=torch.float64, device=d)
    cache[:, 0] = -1
    nxt = torch.empty_like(ts)
    snap = torch.zeros((B, dev.snapshot_doubles), dtype=torch.float64, device=d)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = _native._ptr
    L = _native.lib()
    _native._check(L.nimble_forward_pw(dev.h, B, p(ts), p(tf), p(cache), p(nxt), p(snap), C.c_void_p(0), stream))
    gs, gf = torch.empty_like(ts), torch.empty_like(tf)
    gi = torch.empty((B, dev.nb, 10), dtype=torch.float64, device=d)
    _native._check(L.nimble_backward_inertia_pw(dev.h, B, p(ts), p(tf), p(snap), p(tg), p(gs), p(gf), p(gi),
                                                C.c_void_p(0), stream))
    torch.cuda.synchronize()
    ref = dict(zip(OUTPUTS, shared[0]))
    assert torch.equal(nxt, ref["next state"]) and torch.equal(cache, ref["LCP cache"])
    assert torch.equal(gs, ref["grad state"]) and torch.equal(gf, ref["grad forces"])
    assert torch.equal(gi, ref["grad inertia"])
    # and None through the wrapper (what _run does for the shared path)
    again = _run(world, st, f, g, bi=None)
    _assert_rows_equal("None", again, shared[0], list(range(B)))


@pytest.mark.parametrize("name", sorted(MODELS))
def test_per_world_equals_one_model_per_parameter_set(name):
    """Test 2: one per-world run with all three sets against three
    shared-model runs, each on a device model built with one set."""
    world, st, f, g, shared, own, per = _results(name)
    B = st.shape[0]
    for k in range(PW.K):
        _assert_rows_equal(f"{name} set {k}", per, shared[k], [b for b in range(B) if b % PW.K == k])
    # the sets do change the step (the comparison is not between equal inputs)
    assert not torch.equal(per[0][1], shared[0][0][1])
    if name == "atlas_contact":
        m = dict(zip(OUTPUTS, per))["snapshot header"][:, SN_M]
        # >= 12 rows: the backward's pool is in the HBM workspace
        assert bool((m >= 12).any()) and bool((m < 12).any()), m.tolist()


def _mesh_check():
    world, st, f, g, shared, own, per = _results("atlas_mesh", mesh=True)
    B = st.shape[0]
    m = dict(zip(OUTPUTS, per))["snapshot header"][:, SN_M].tolist()
    assert m[MESH_WIDE_WORLD] > 64 and max(m[:MESH_WIDE_WORLD]) <= 64 and B <= 32, m
    assert all(int(s) & _native.ST_DIVERGES == 0 for s in dict(zip(OUTPUTS, per))["snapshot header"][:, SN_STATUS])
    _assert_rows_equal("atlas_mesh own", own, shared[0], list(range(B)))
    for k in range(PW.K):
        _assert_rows_equal(f"atlas_mesh set {k}", per, shared[k], [b for b in range(B) if b % PW.K == k])
    return m


def test_wide_kernels_mesh_atlas():
    """Test 3: the STL-mesh Atlas; the world with more than 64 LCP rows takes
    the wide forward and nimble_backward_wide_kernel (row count asserted from
    the snapshot header)."""
    _mesh_check()


def test_wide_kernels_mesh_atlas_defer_rows_0():
    """Test 3 once more with NIMBLE_AMD_DEFER_ROWS=0 (every world with LCP
    rows through the two-rows-per-lane kernels), in a fresh process: the
    threshold is read when the library first builds a device model."""
    env = dict(os.environ)
    env["NIMBLE_AMD_DEFER_ROWS"] = "0"
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")])
    r = subprocess.run([sys.executable, "-c", "import test_gpu_per_world_inertia as t; print('rows', t._mesh_check())"],
                       env=env, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "rows" in r.stdout


def test_three_step_rollout():
    """Test 4: Atlas in contact, three chained steps (state and LCP cache fed
    back): the warm start and the caches under differing parameters."""
    world, st0, f, g, _, _, _ = _results("atlas_contact")
    B = st0.shape[0]
    sets = PW.param_sets(world)

    def rollout(bi):
        st, cache, out = st0, None, []
        for _ in range(3):
            r = _run(world, st, f, g, bi=bi, cache=cache)
            out.append(r)
            st, cache = r[0].cpu().numpy(), r[1]
        return out

    per = rollout(PW.batch_params(world, B))
    for k in (1, 2, 0):
        PW.set_world_params(world, sets[k])
        ref = rollout(None)
        for step in range(3):
            _assert_rows_equal(f"step {step} set {k}", per[step], ref[step], [b for b in range(B) if b % PW.K == k])
    assert not torch.equal(per[2][0], per[0][0])


@pytest.mark.parametrize("name,bodies", [("cartpole", [0, 1]), ("atlas_air", [5, 20])])
def test_oracle_parity_without_lcp(name, bodies):
    """Test 5: no contact, so no LCP path to split: the oracle built from the
    Python world set to each world's parameters.  Next state within 1e-12
    absolute, state / force gradients within 1e-9 of the largest reference
    entry (the bounds of test_box_step_emulated), and grad_inertia of two
    bodies against central differences of that oracle step (step sizes,
    1e-6 bound and noise floor of test_gpu_mass._inertia_parity)."""
    world, st, f, g, shared, own, per = _results(name)
    B = st.shape[0]
    sets = PW.param_sets(world)
    out = {k: v.cpu().numpy() for k, v in zip(OUTPUTS, per)}
    blist = [b for s in world.skeletons for b in s.bodies]
    index = {id(e[2]): i for i, e in enumerate(world._model_bodies()) if e[2] is not None}
    try:
        for k in range(PW.K):
            rows = [b for b in range(B) if b % PW.K == k]
            PW.set_world_params(world, sets[k])
            ow = O.OracleWorld(world)
            ref = ow.forward(st, f)
            rgs, rgf = ow.backward(g)
            err = np.abs(out["next state"][rows] - ref[rows]).max()
            egs = np.abs(out["grad state"][rows] - rgs[rows]).max() / np.abs(rgs[rows]).max()
            egf = np.abs(out["grad forces"][rows] - rgf[rows]).max() / np.abs(rgf[rows]).max()
            print(f"{name} set {k}: next-state abs err {err:.3e}, grad state {egs:.3e}, grad forces {egf:.3e}")
            assert err <= 1e-12 and egs <= 1e-9 and egf <= 1e-9, (k, err, egs, egf)
            got, cd, noise = [], [], []
            for bi in bodies:
                body = blist[bi]
                for p in range(10):
                    v0 = _get_param(body, p)
                    e = 1e-6 * max(abs(v0), 1e-2)
                    try:
                        _set_param(body, p, v0 + e)
                        lp = (O.OracleWorld(world).forward(st, f) * g).sum(axis=1)
                        _set_param(body, p, v0 - e)
                        lm = (O.OracleWorld(world).forward(st, f) * g).sum(axis=1)
                    finally:
                        _set_param(body, p, v0)
                    got.append(out["grad inertia"][rows, index[id(body)], p])
                    cd.append(((lp - lm) / (2 * e))[rows])
                    noise.append(1e-14 * np.abs(lp).max() / e)
            got, cd = np.stack(got, axis=1), np.stack(cd, axis=1)
            gerr = np.abs(got - cd)
            bound = 1e-6 * np.abs(cd).max() + 3 * np.array(noise)[None, :]
            print(f"{name} set {k}: grad_inertia max err {gerr.max():.3e} of {np.abs(cd).max():.3e}")
            assert (gerr <= bound).all(), (k, gerr.max(axis=0), np.abs(cd).max(axis=0), noise)
    finally:
        PW.set_world_params(world, sets[0])


def _tuned_atlas():
    w = models.atlas_world(True)
    w.setStatusPolicy("record")
    bodies = [b for s in w.skeletons for b in s.bodies]
    bodies[27].setBeta([1.0, 0.5, 0.0])
    bodies[27].setLocalCOM(bodies[27].getBeta() * 0.03)
    w.tuneMass(bodies[0], "INERTIA_MASS")
    w.tuneMass(bodies[27], "INERTIA_COM_MU")
    w.tuneMass(bodies[30], "INERTIA_DIAGONAL")
    w.tuneMass(bodies[5], "INERTIA_FULL")
    st, f = models.random_states(w, 6, seed=8, q_scale=0.01, v_scale=0.02)
    m0 = w.getMasses()
    rows = np.stack([m0 * (1.0, 0.9, 1.15)[b % 3] for b in range(6)])
    return w, st, f, m0, rows


def test_timestep_two_dimensional_mass():
    """Test 6, autograd: timestep with a [B, D] mass; mass.grad [B, D] is the
    shared path's mass_gradient per parameter set, row by row, before its
    batch sum; the world object is left alone."""
    import nimblephysics_amd as nimble
    w, st, f, m0, rows = _tuned_atlas()
    d = torch.device("cuda:0")
    B, D = rows.shape
    g = np.random.default_rng(1).standard_normal(st.shape)
    tg = torch.tensor(g, device=d)
    mass = torch.tensor(rows, device=d, requires_grad=True)
    ts = torch.tensor(st, device=d, requires_grad=True)
    tf = torch.tensor(f, device=d, requires_grad=True)
    dev0, version = w.native(), w._version
    out = nimble.timestep(w, ts, tf, mass)
    out.backward(tg)
    assert tuple(mass.grad.shape) == (B, D)
    assert w._version == version and np.array_equal(w.getMasses(), m0) and w.native() is dev0
    stream = torch.cuda.current_stream().cuda_stream
    try:
        for k in range(3):
            sel = [b for b in range(B) if b % 3 == k]
            w.setMasses(rows[k])
            w._batch_state = None
            dev, forces, nxt, snap = step_batch(w, ts.detach(), tf.detach())
            gs, gf = torch.empty_like(nxt), torch.empty_like(forces)
            gm = mass_gradient(dev, w._mass_selection(), ts.detach(), forces, snap, tg, gs, gf, stream)
            torch.cuda.synchronize()
            assert torch.equal(out.detach()[sel], nxt[sel])
            assert torch.equal(ts.grad[sel], gs[sel]) and torch.equal(tf.grad[sel], gf[sel])
            assert np.allclose(mass.grad[sel].cpu().numpy(), gm[sel].cpu().numpy(), rtol=1e-12, atol=0), k
        assert not torch.equal(mass.grad[0], mass.grad[1])
    finally:
        w.setMasses(m0)
    # shape errors
    with pytest.raises(ValueError):
        nimble.timestep(w, ts[0], tf[0], mass)
    with pytest.raises(ValueError):
        nimble.timestep(w, ts, tf, mass[:B - 1])
    with pytest.raises(ValueError):
        nimble.timestep(w, ts, tf, mass[:, :D - 1])
    with pytest.raises(ValueError):
        neural.forwardPass(w, state=ts, action=tf, mass=mass[:, :D - 1])


def test_forward_pass_snapshot_keeps_the_parameters():
    """Test 6, neural: forwardPass(..., mass=) and the snapshot's Jacobians,
    dF_c and backpropState are each world's own model's."""
    w, st, f, m0, rows = _tuned_atlas()
    d = torch.device("cuda:0")
    B, D = rows.shape
    ts, tf = torch.tensor(st, device=d), torch.tensor(f, device=d)
    tg = torch.tensor(np.random.default_rng(3).standard_normal(st.shape), device=d)
    w._batch_state = None
    snap = neural.forwardPass(w, state=ts, action=tf, mass=torch.tensor(rows, device=d))
    J = snap.getStateJacobian(w)
    A = snap.getActionJacobian(w)
    dfc = snap.getJacobianOfConstraintForce(w, "FORCE")
    bp = snap.backpropState(w, tg)
    assert tuple(bp.lossWrtMass.shape) == (B, D)
    assert np.array_equal(w.getMasses(), m0)
    try:
        for k in range(3):
            sel = [b for b in range(B) if b % 3 == k]
            w.setMasses(rows[k])
            w._batch_state = None
            ref = neural.forwardPass(w, state=ts, action=tf)
            assert torch.equal(snap.getPostStepPosition()[sel], ref.getPostStepPosition()[sel])
            assert torch.equal(J[sel], ref.getStateJacobian(w)[sel])
            assert torch.equal(A[sel], ref.getActionJacobian(w)[sel])
            assert torch.equal(dfc[sel], ref.getJacobianOfConstraintForce(w, "FORCE")[sel])
            rb = ref.backpropState(w, tg)
            assert torch.equal(bp.lossWrtState[sel], rb.lossWrtState[sel])
            assert torch.equal(bp.lossWrtAction[sel], rb.lossWrtAction[sel])
            assert np.allclose(bp.lossWrtMass[sel].cpu().numpy(), rb.lossWrtMass[sel].cpu().numpy(), rtol=1e-12, atol=0)
        assert bool((snap.getNumClamping() > 0).any())
    finally:
        w.setMasses(m0)
