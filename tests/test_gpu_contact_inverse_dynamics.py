"""Batched contact inverse dynamics on the GPU: nimble_contact_inverse_dynamics,
DeviceWorld.contact_inverse_dynamics, the Python layer
(nimblephysics_amd.contact_inverse_dynamics) and the Skeleton methods
(getContactInverseDynamics, getMultipleContactInverseDynamics).

1. Values against the numpy restatement of the reference's formulas
   (contact_invdyn_refs.reference: the KKT system with np.linalg.solve without
   guesses, np.linalg.pinv with them -- not the kernel's closed form), fed with
   tau_full from the oracle (invdyn_refs.Ref.tau) and the stacked body-frame
   Jacobians from the existing backward (grad_tau = e_j: body-frame grad_wrench
   is -J[:, j]).  The test asserts cond(N) <= 1e8 on its inputs.
2. Physics closure, independent of 1 (the reference's sumError): the existing
   step with tau and the contact wrenches has v' = v + dt a; shared model,
   per-world mass [B, D], a known extra body_wrench in each frame; the root
   rows are exactly 0.0.
3. Selection: guesses that already satisfy the root equation come back; one
   body gives the same wrench with and without a guess; 1-D against row 0 of
   2-D bit for bit; the CPU-tensor round trip.
4. The Skeleton methods against the functional call at the world's state, with
   a stored wrench on a non-contact body; sumError() <= 1e-9 max(1, |a|).

Bar everywhere: RTOL = 1e-6 under _rel with floor 1e-5.  B = 3.

Results before this feature: FEATURE MISSING -- the entry point, the
DeviceWorld method, nimblephysics_amd.contact_inverse_dynamics and the Skeleton
methods do not exist, so every test here fails on the parent commit.

Observed maxima on the MI355X under _rel (each test prints its figures before
it asserts; DESIGN.md, "Contact inverse dynamics" under Kernels, has the same):
    1 values          tau 6.2e-12, contact wrenches 2.4e-12 (Atlas, feet + l_hand
                      with guesses / eight bodies); the rig 4.0e-14 / 3.6e-13,
                      with another skeleton first 6.4e-14 / 2.5e-13, the Atlas
                      on the ground in contact 7.8e-13 / 3.6e-13; the numpy
                      cond(N) at most 4.3e+02
    2 closure         v' = v + dt a to 3.2e-12 (Atlas, feet), extra wrench body
                      1.8e-12 / world 2.2e-12; per-world mass 2.7e-14
    3 selection       feasible guesses come back to 3.6e-14; k = 1 with and
                      without a guess 9.1e-14 (tau 2.9e-13)
    4 Skeleton        equal to the functional call bit for bit; sumError
                      1.7e-11, 5.0e-13, 4.4e-13 against the bar 1.3e-08
"""
import functools

import numpy as np
import pytest
import torch

import contact_invdyn_refs as cref
import invdyn_refs
import models
import nimblephysics_amd as nimble
from nimblephysics_amd.contact_inverse_dynamics import contact_body_indices
from oracle import oracle as O
from test_gpu_contact_parity import RTOL, _rel

pytestmark = pytest.mark.gpu

B = 3
D = "cuda:0"

ATLAS_8 = ["l_foot", "r_foot", "l_hand", "r_hand", "pelvis", "utorso", "l_lleg", "r_uarm"]
# model -> (world kind, contact body names)
CASES = {
    "rig": ("rig", ["l_foot", "r_foot", "arm"]),
    "atlas_feet": ("atlas_air", ["l_foot", "r_foot"]),
    "atlas_feet_hand": ("atlas_air", ["l_foot", "r_foot", "l_hand"]),
    "atlas_8": ("atlas_air", ATLAS_8),
    "atlas_ground": ("atlas_contact", ["l_foot", "r_foot"]),
    "rig_second": ("rig_second", ["r_foot", "l_foot"]),
}


def _t(x):
    return None if x is None else torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=D)


def _np(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _world(kind):
    """World, states, accelerations and the oracle's tau_full, made once per
    world and left unchanged."""
    if kind in ("rig", "rig_second"):
        w = cref.rig_world(fixed_first=kind == "rig_second")
        st, a = cref.rig_states(w, B, seed=11)
    elif kind == "atlas_air":
        w = models.atlas_world(False)
        st, _ = models.random_states(w, B, seed=3, q_scale=0.2, v_scale=0.3)
        a = invdyn_refs.accelerations((B, w.getNumDofs()), seed=5)
    else:  # the Atlas on the ground, at states in contact
        assert kind == "atlas_contact"
        w = models.atlas_world(True)
        st, _ = models.random_states(w, 8 * B, seed=3, q_scale=0.01, v_scale=0.02)
        counts, _ = O.OracleWorld(w).detect(st)
        st = st[counts > 0][:B]
        assert st.shape[0] == B
        a = invdyn_refs.accelerations((B, w.getNumDofs()), seed=5)
    w.setStatusPolicy("record")
    ref = invdyn_refs.Ref(w)
    return w, st, a, ref, ref.tau_batch(st, a)


def _rig_skeleton(world):
    """(the skeleton with the free root, the first of its dofs)"""
    r0 = 0
    for s in world.skeletons:
        if s.bodies[0].joint.kind == 3:
            return s, r0
        r0 += s.getNumDofs()
    raise AssertionError("no free root")


def _bodies(world, names):
    skel, _ = _rig_skeleton(world)
    return [skel.getBodyNode(x) for x in names]


@functools.lru_cache(maxsize=None)
def _jacobians(kind):
    """Body-frame Jacobians of every device-model body, [B, nb, 6, n], from the
    existing backward: one item per (world, dof) with grad_tau = e_dof and a
    zero body-frame wrench; grad_wrench is minus the Jacobian's column."""
    world, st, a, _, _ = _world(kind)
    dev = world.native()
    n, nb = dev.n, dev.nb
    st2, a2 = np.repeat(st, n, axis=0), np.repeat(a, n, axis=0)
    g2 = np.tile(np.eye(n), (B, 1))
    gs = torch.empty((B * n, 2 * n), dtype=torch.float64, device=D)
    ga = torch.empty((B * n, n), dtype=torch.float64, device=D)
    gw = torch.full((B * n, nb, 6), float("nan"), dtype=torch.float64, device=D)
    dev.inverse_dynamics_backward(_t(st2), _t(a2), _t(g2), gs, ga, torch.cuda.current_stream().cuda_stream,
                                  body_wrench=torch.zeros_like(gw), wrench_frame="body", grad_wrench=gw)
    torch.cuda.synchronize()
    return -np.transpose(_np(gw).reshape(B, n, nb, 6), (0, 2, 3, 1))


def _guesses(k, seed=13):
    return 20.0 * np.random.default_rng(seed).standard_normal((B, k, 6))


# --- 1. values ---------------------------------------------------------------------
@pytest.mark.parametrize("guess", [False, True], ids=["smallest_moments", "nearest_guess"])
@pytest.mark.parametrize("case", list(CASES))
def test_values_against_the_reference_formulas(case, guess):
    kind, names = CASES[case]
    world, st, a, ref, tau_full = _world(kind)
    n = world.getNumDofs()
    skel, r0 = _rig_skeleton(world)
    bodies = _bodies(world, names)
    idx = contact_body_indices(world, bodies)
    k = len(idx)
    if case == "atlas_ground":
        counts, _ = ref.o.detect(st)
        assert (counts > 0).all() and world.native().num_pairs > 0  # in contact: and contacts play no part
    if case == "atlas_8":
        assert k == 8 and len(set(idx)) == 8
    if case == "rig_second":
        assert r0 == 2
    J = _jacobians(kind)
    F0 = _guesses(k) if guess else None
    tau, F = nimble.contact_inverse_dynamics(world, _t(st), _t(a), bodies, wrench_guesses=_t(F0))
    tau, F = _np(tau), _np(F)
    rt, rF, conds = np.zeros_like(tau), np.zeros_like(F), []
    for b in range(B):
        rt[b], rF[b], c = cref.reference(tau_full[b], J[b, idx].reshape(6 * k, n), r0, None if F0 is None else F0[b])
        conds.append(c)
    e = {"tau": _rel(tau, rt), "F": _rel(F, rF)}
    print(case, "guess" if guess else "no guess", {key: f"{v:.2e}" for key, v in e.items()},
          f"cond(N) {max(conds):.1e}")
    assert max(conds) <= 1e8, conds
    assert np.all(tau[:, r0:r0 + 6] == 0.0) and not np.any(np.signbit(tau[:, r0:r0 + 6]))
    assert np.abs(F).max() > 1.0
    if case == "rig_second":
        # the pendulum's torques are plain inverse dynamics, bit for bit
        plain = _np(nimble.inverse_dynamics(world, _t(st), _t(a)))
        assert np.array_equal(tau[:, :2], plain[:, :2]) and np.abs(plain[:, :2]).min() > 0
        assert not np.array_equal(tau[:, 8:], plain[:, 8:])
    for key, v in e.items():
        assert v <= RTOL, (case, guess, key, v)


# --- 2. physics closure ---------------------------------------------------------------
def _scatter(world, bodies, F):
    """Contact wrenches [B, k, 6] as a body_wrench [B, getNumBodyNodes(), 6]."""
    order = {id(b): i for i, b in enumerate(world._world_bodies())}
    W = torch.zeros((F.shape[0], world.getNumBodyNodes(), 6), dtype=torch.float64, device=F.device)
    for i, b in enumerate(bodies):
        W[:, order[id(b)]] = F[:, i]
    return W


@pytest.mark.parametrize("case", ["rig", "atlas_feet", "atlas_feet_hand", "rig_second"])
def test_the_step_under_tau_and_the_wrenches_has_the_accelerations(case):
    kind, names = CASES[case]
    world, st, a, ref, _ = _world(kind)
    n = world.getNumDofs()
    skel, r0 = _rig_skeleton(world)
    bodies = _bodies(world, names)
    ts, ta = _t(st), _t(a)
    want = st[:, n:] + ref.dt * a
    e = {}
    for guess in (False, True):
        F0 = _t(_guesses(len(bodies))) if guess else None
        tau, F = nimble.contact_inverse_dynamics(world, ts, ta, bodies, wrench_guesses=F0)
        assert torch.all(tau[:, r0:r0 + 6] == 0.0)
        nxt = nimble.timestep(world, ts, tau, body_wrench=_scatter(world, bodies, F), wrench_frame="body")
        e["guess" if guess else "no guess"] = _rel(_np(nxt)[:, n:], want)
    # a known extra wrench on every body: in body frame it adds to the contact
    # wrenches; in world frame the step's linearity in the wrenches takes it in:
    # v'(tau, F + extra) = v'(tau, F) + v'(0, extra) - v'(0, 0)
    extra = _t(2.0 * np.random.default_rng(14).standard_normal((B, world.getNumBodyNodes(), 6)))
    zero = torch.zeros_like(ta)
    free = nimble.timestep(world, ts, zero)
    for frame in ("body", "world"):
        tau, F = nimble.contact_inverse_dynamics(world, ts, ta, bodies, body_wrench=extra, wrench_frame=frame)
        assert torch.all(tau[:, r0:r0 + 6] == 0.0)
        Fw = _scatter(world, bodies, F)
        if frame == "body":
            nxt = nimble.timestep(world, ts, tau, body_wrench=Fw + extra, wrench_frame="body")
        else:
            nxt = (nimble.timestep(world, ts, tau, body_wrench=Fw, wrench_frame="body")
                   + nimble.timestep(world, ts, zero, body_wrench=extra, wrench_frame="world") - free)
        e["extra " + frame] = _rel(_np(nxt)[:, n:], want)
    print(case, {key: f"{v:.2e}" for key, v in e.items()})
    for key, v in e.items():
        assert v <= RTOL, (case, key, v)


def test_closure_with_per_world_mass():
    world = cref.rig_world()
    skel = world.getSkeleton("rig")
    for name in ("torso", "l_shin", "r_foot"):
        world.tuneMass(skel.getBodyNode(name), "INERTIA_MASS")
    m0 = world.getMasses().copy()
    st, a = cref.rig_states(world, B, seed=11)
    n = world.getNumDofs()
    ts, ta = _t(st), _t(a)
    m2 = torch.tensor(np.stack([m0 * s for s in (0.6, 1.0, 1.7)]), device=D)
    bodies = [skel.getBodyNode("l_foot"), skel.getBodyNode("r_foot")]
    tau, F = nimble.contact_inverse_dynamics(world, ts, ta, bodies, mass=m2)
    own, Fown = nimble.contact_inverse_dynamics(world, ts, ta, bodies)
    assert torch.all(tau[:, :6] == 0.0)
    # row 1 has the model's own masses; the others differ from it
    assert _rel(_np(tau[1]), _np(own[1])) <= RTOL and _rel(_np(F[1]), _np(Fown[1])) <= RTOL
    assert _rel(_np(tau[0]), _np(own[0])) > 1e-2 and _rel(_np(F[2]), _np(Fown[2])) > 1e-2
    nxt = nimble.timestep(world, ts, tau, mass=m2, body_wrench=_scatter(world, bodies, F), wrench_frame="body")
    err = _rel(_np(nxt)[:, n:], st[:, n:] + world.getTimeStep() * a)
    one, Fone = nimble.contact_inverse_dynamics(world, ts, ta, bodies, mass=m2[2])
    print(f"per-world mass closure {err:.2e}")
    assert err <= RTOL, err
    assert torch.equal(one[2], tau[2]) and torch.equal(Fone[2], F[2]) and np.array_equal(world.getMasses(), m0)


# --- 3. selection properties ------------------------------------------------------------
def test_selection_properties():
    world, st, a, ref, _ = _world("atlas_air")
    n = world.getNumDofs()
    bodies = _bodies(world, ["l_foot", "r_foot", "l_hand"])
    ts, ta = _t(st), _t(a)
    e = {}
    # guesses that already satisfy the root equation come back: the wrenches of
    # one solution are such guesses
    tau0, Fa = nimble.contact_inverse_dynamics(world, ts, ta, bodies)
    tau1, Fb = nimble.contact_inverse_dynamics(world, ts, ta, bodies, wrench_guesses=Fa)
    e["feasible guess F"] = _rel(_np(Fb), _np(Fa))
    e["feasible guess tau"] = _rel(_np(tau1), _np(tau0))
    # ... and infeasible ones do not, and give another solution of the same motion
    _, Fc = nimble.contact_inverse_dynamics(world, ts, ta, bodies, wrench_guesses=_t(_guesses(3)))
    assert _rel(_np(Fc), _np(Fa)) > 1e-2
    # one body determines its wrench
    one = bodies[:1]
    t1, F1 = nimble.contact_inverse_dynamics(world, ts, ta, one)
    t2, F2 = nimble.contact_inverse_dynamics(world, ts, ta, one, wrench_guesses=_t(_guesses(1)))
    e["k = 1 F"] = _rel(_np(F2), _np(F1))
    e["k = 1 tau"] = _rel(_np(t2), _np(t1))
    print({key: f"{v:.2e}" for key, v in e.items()})
    for key, v in e.items():
        assert v <= RTOL, (key, v)
    # 1-D against row 0 of 2-D, bit for bit; the CPU round trip; detached outputs
    G = _t(_guesses(3))
    tau2, F2d = nimble.contact_inverse_dynamics(world, ts, ta, bodies, wrench_guesses=G)
    tau1d, F1d = nimble.contact_inverse_dynamics(world, ts[0], ta[0], bodies, wrench_guesses=G[0])
    assert tau1d.shape == (n,) and F1d.shape == (3, 6)
    assert torch.equal(tau1d, tau2[0]) and torch.equal(F1d, F2d[0])
    before = (world.getState().copy(), world._version)
    sc, ac = ts.cpu().requires_grad_(True), ta.cpu().requires_grad_(True)
    tauc, Fcpu = nimble.contact_inverse_dynamics(world, sc, ac, bodies, wrench_guesses=G.cpu())
    assert tauc.device.type == "cpu" and Fcpu.device.type == "cpu"
    assert not tauc.requires_grad and not Fcpu.requires_grad
    assert torch.equal(tauc.to(D), tau2) and torch.equal(Fcpu.to(D), F2d)
    assert np.array_equal(world.getState(), before[0]) and world._version == before[1]
    # the differentiable route the docstring names gives the same torques
    # outside the root rows
    Wd = _scatter(world, bodies, F2d)
    full = nimble.inverse_dynamics(world, ts, ta, body_wrench=Wd, wrench_frame="body")
    assert _rel(_np(full)[:, 6:], _np(tau2)[:, 6:]) <= RTOL
    assert np.abs(_np(full)[:, :6]).max() <= 1e-9 * np.abs(_np(tau2)).max()


# --- 4. the Skeleton methods -----------------------------------------------------------
def test_skeleton_methods():
    world = cref.rig_world(fixed_first=True)
    rig, pend = world.getSkeleton("rig"), world.getSkeleton("pendulum")
    st, a = cref.rig_states(world, 1, seed=23)
    n, ns = world.getNumDofs(), rig.getNumDofs()
    lo = pend.getNumDofs()
    world.setState(st[0])
    acc = a[0, lo:]
    stored = np.array([0.3, -0.2, 0.1, 1.5, -2.0, 0.7])
    rig.getBodyNode("l_thigh").setExtWrench(stored)
    lf, rf, arm = rig.getBodyNode("l_foot"), rig.getBodyNode("r_foot"), rig.getBodyNode("arm")
    W = np.zeros((world.getNumBodyNodes(), 6))
    W[world._world_bodies().index(rig.getBodyNode("l_thigh"))] = stored
    a_world = np.concatenate([np.zeros(lo), acc])
    ts, ta, tw = _t(st[0]), _t(a_world), _t(W)
    bar = 1e-9 * max(1.0, float(np.linalg.norm(acc)))
    # one body
    res = rig.getContactInverseDynamics(acc, lf)
    tau, F = nimble.contact_inverse_dynamics(world, ts, ta, [lf], body_wrench=tw, wrench_frame="body")
    assert res.skel is rig and res.contactBody is lf
    assert np.array_equal(res.pos, st[0, lo:n]) and np.array_equal(res.vel, st[0, n + lo:])
    assert np.array_equal(res.acc, acc)
    assert res.jointTorques.shape == (ns,) and res.contactWrench.shape == (6,)
    assert np.array_equal(res.jointTorques, _np(tau)[lo:]) and np.array_equal(res.contactWrench, _np(F)[0])
    assert np.all(res.jointTorques[:6] == 0.0)
    errs = [res.sumError()]
    # the stored wrench was applied, and stays stored
    plain, _ = nimble.contact_inverse_dynamics(world, ts, ta, [lf])
    assert not np.array_equal(_np(plain)[lo:], res.jointTorques)
    assert np.array_equal(rig.getBodyNode("l_thigh").getExternalForceLocal(), stored)
    # several bodies, without and with guesses
    many = rig.getMultipleContactInverseDynamics(acc, [lf, rf, arm])
    tau, F = nimble.contact_inverse_dynamics(world, ts, ta, [lf, rf, arm], body_wrench=tw, wrench_frame="body")
    assert many.contactBodies == [lf, rf, arm] and many.contactWrenchGuesses == []
    assert np.array_equal(many.jointTorques, _np(tau)[lo:])
    assert all(np.array_equal(many.contactWrenches[i], _np(F)[i]) for i in range(3))
    errs.append(many.sumError())
    G = _guesses(3, seed=29)[0]
    near = rig.getMultipleContactInverseDynamics(acc, [lf, rf, arm], [g for g in G])
    tau, F = nimble.contact_inverse_dynamics(world, ts, ta, [lf, rf, arm], wrench_guesses=_t(G), body_wrench=tw,
                                             wrench_frame="body")
    assert np.array_equal(near.jointTorques, _np(tau)[lo:]) and np.array_equal(np.stack(near.contactWrenches), _np(F))
    assert np.array_equal(np.stack(near.contactWrenchGuesses), G)
    assert not np.array_equal(near.jointTorques, many.jointTorques)
    errs.append(near.sumError())
    print("sumError", [f"{x:.2e}" for x in errs], f"bar {bar:.2e}")
    assert max(errs) <= bar, (errs, bar)
    # a wrong answer is seen by sumError
    near.jointTorques = near.jointTorques + 1e-3
    assert near.sumError() > 1e3 * bar
    assert np.array_equal(world.getState(), st[0])
