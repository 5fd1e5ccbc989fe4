"""Batched differentiable inverse dynamics on the GPU: nimble_inverse_dynamics
/ nimble_inverse_dynamics_backward, DeviceWorld.inverse_dynamics*, and the
Python layer (inverse_dynamics, mass_matrix, coriolis_and_gravity, the World
getters).

References (tests/invdyn_refs.py, all CPU, none from the code under test):
values from the oracle's mass matrix and bias force; gradients from the
oracle's analytic step Jacobian turned into the Jacobian of ID, and from
Richardson-extrapolated central differences (tests/test_inverse_dynamics_host.py
holds the two to each other ten times inside the bar); the wrench terms from
numpy on the Tw / Sw the existing shared forward caches
(tests/test_gpu_body_wrench.py); and the existing forward itself, which tau
must invert.  Bar everywhere: RTOL = 1e-6 under _rel with floor 1e-5.

Results before this feature: FEATURE MISSING -- the entry points, the
DeviceWorld methods and nimblephysics_amd.inverse_dynamics do not exist, so
every test here fails on the parent commit.

Observed maxima on the MI355X under _rel (each test prints its figures before
it asserts; DESIGN.md, "Inverse dynamics" under Kernels, has the same):
    1 values          tau 3.7e-13, mass_matrix 1.7e-11, bias 1.3e-12
                      (Atlas on the ground in contact: 2.9e-13, 1.5e-11, 3.7e-13)
    2 round trip      1.3e-13 (no wrench 7.3e-14, world 8.2e-14, body 1.3e-13)
    3 VJP             grad_state 1.6e-9 (ball rig), grad_ddq 1.4e-11
    4 wrenches        tau 2.2e-14, grad_wrench 3.7e-14, grad_state 3.0e-8 against
                      the Richardson reference (itself within 1.3e-8 of the
                      analytic one, tests/test_inverse_dynamics_host.py)
    5 per-world       tau 2.8e-13, mass_matrix 1.3e-11, bias 3.3e-13
    6 autograd        equal to the C-ABI outputs bit for bit; slope dt to 4.6e-13
"""
import functools

import numpy as np
import pytest
import torch

import invdyn_refs
import models
import nimblephysics_amd as nimble
import per_world_params as PW
from oracle import oracle as O
from test_gpu_body_wrench import _body_twists, _forward_kin, _tau_ext, _to_frame, _to_world, _tree, _wrenches
from test_gpu_contact_parity import RTOL, _rel

pytestmark = pytest.mark.gpu

B = 3
FRAMES = ("world", "body")
D = "cuda:0"


def _t(x):
    return None if x is None else torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=D)


def _states(name, batch):
    if name == "cartpole":
        w = invdyn_refs.damped_cartpole()
        st, _ = models.random_states(w, batch, seed=3, q_scale=0.5, v_scale=1.0)
    elif name == "kr5":
        w = models.kr5_world()
        st, _ = models.random_states(w, batch, seed=3, q_scale=0.5, v_scale=1.0)
    elif name == "ball":
        w = models.ball_world(ground=False)
        st, _ = models.ball_states(batch, seed=21, contact=False)
    elif name == "compound":
        w = models.compound_world(ground=False)
        st, _ = models.compound_states(batch, seed=21, contact=False)
    elif name == "atlas_air":
        w = models.atlas_world(False)
        st, _ = models.random_states(w, batch, seed=3, q_scale=0.2, v_scale=0.3)
    else:  # the Atlas on the ground, at states in contact
        assert name == "atlas_contact"
        w = models.atlas_world(True)
        st, _ = models.random_states(w, 8 * batch, seed=3, q_scale=0.01, v_scale=0.02)
        counts, _ = O.OracleWorld(w).detect(st)
        st = st[counts > 0][:batch]  # (the sampler's worlds that touch the ground)
        assert st.shape[0] == batch
    w.setStatusPolicy("record")
    return w, st


FREE = ("cartpole", "kr5", "ball", "compound", "atlas_air")  # no collision pairs


@functools.lru_cache(maxsize=None)
def _case(name, batch=B):
    """World, states, accelerations and the oracle references, made once per
    model and left unchanged."""
    world, st = _states(name, batch)
    n = world.getNumDofs()
    a = invdyn_refs.accelerations((batch, n), seed=5)
    ref = invdyn_refs.Ref(world)
    return world, st, a, ref, ref.tau_batch(st, a)


@functools.lru_cache(maxsize=None)
def _analytic(name):
    """Per world (dID/dq, dID/dv, dID/da) from the oracle's analytic step
    Jacobian."""
    world, st, a, ref, _ = _case(name)
    n = world.getNumDofs()
    return [ref.analytic(st[b, :n], st[b, n:], a[b]) for b in range(st.shape[0])]


@functools.lru_cache(maxsize=None)
def _richardson(name):
    """Per world (dID/dq, dID/dv, dID/da) by Richardson differences of the
    oracle's tau."""
    world, st, a, ref, _ = _case(name)
    n = world.getNumDofs()
    return [ref.richardson(st[b, :n], st[b, n:], a[b]) for b in range(st.shape[0])]


def _id(world, st, a, bi=None, bw=None, frame="world", extras=True):
    """(tau, mass_matrix, bias) through DeviceWorld.inverse_dynamics."""
    dev = world.native()
    Bn, n = st.shape[0], dev.n
    ts, ta = _t(st), _t(a)
    tau = torch.full((Bn, n), float("nan"), dtype=torch.float64, device=D)
    M = torch.full((Bn, n, n), float("nan"), dtype=torch.float64, device=D) if extras else None
    C = torch.full((Bn, n), float("nan"), dtype=torch.float64, device=D) if extras else None
    dev.inverse_dynamics(ts, ta, tau, torch.cuda.current_stream().cuda_stream, body_inertia=_t(bi),
                         body_wrench=_t(bw), wrench_frame=frame, mass_matrix=M, bias=C)
    torch.cuda.synchronize()
    return tau, M, C


def _id_bwd(world, st, a, g, bi=None, bw=None, frame="world", want_gw=False):
    """(grad_state, grad_ddq, grad_wrench) through DeviceWorld.inverse_dynamics_backward."""
    dev = world.native()
    Bn, n = st.shape[0], dev.n
    gs = torch.full((Bn, 2 * n), float("nan"), dtype=torch.float64, device=D)
    ga = torch.full((Bn, n), float("nan"), dtype=torch.float64, device=D)
    gw = torch.full((Bn, dev.nb, 6), float("nan"), dtype=torch.float64, device=D) if want_gw else None
    dev.inverse_dynamics_backward(_t(st), _t(a), _t(g), gs, ga, torch.cuda.current_stream().cuda_stream,
                                  body_inertia=_t(bi), body_wrench=_t(bw), wrench_frame=frame, grad_wrench=gw)
    torch.cuda.synchronize()
    return gs, ga, gw


def _forward(world, st, f, bw=None, frame="world"):
    """Next state of the existing forward (the `_ext` one with wrenches)."""
    dev = world.native()
    Bn = st.shape[0]
    ts, tf = _t(st), _t(f)
    cache = torch.zeros((Bn, dev.cache_doubles), dtype=torch.float64, device=D)
    cache[:, 0] = -1
    nxt = torch.empty_like(ts)
    snap = torch.zeros((Bn, dev.snapshot_doubles), dtype=torch.float64, device=D)
    stream = torch.cuda.current_stream().cuda_stream
    if bw is None:
        dev.forward(ts, tf, cache, nxt, snap, stream)
    else:
        dev.forward(ts, tf, cache, nxt, snap, stream, body_wrench=_t(bw), wrench_frame=frame)
    torch.cuda.synchronize()
    return nxt.cpu().numpy()


def _np(t):
    return t.cpu().numpy()


# --- 1. values ---------------------------------------------------------------------
@pytest.mark.parametrize("name", FREE + ("atlas_contact",))
def test_values_against_the_oracle(name):
    world, st, a, ref, tau_ref = _case(name)
    n = world.getNumDofs()
    if name == "atlas_contact":
        counts, _ = ref.o.detect(st)
        assert (counts > 0).all(), counts  # in contact: and contacts play no part
        assert world.native().num_pairs > 0
    tau, M, C = _id(world, st, a)
    Mref = np.stack([ref.o.mass_matrix(s[:n]) for s in st])
    Cref = np.stack([ref.o.coriolis_gravity(s[:n], s[n:]) for s in st])
    e = {"tau": _rel(_np(tau), tau_ref), "mass_matrix": max(_rel(_np(M)[b], Mref[b]) for b in range(B)),
         "bias": _rel(_np(C), Cref)}
    # without the optional outputs: the same tau
    tau0, _, _ = _id(world, st, a, extras=False)
    assert torch.equal(tau0, tau)
    # B = 1, and the 1-D path of the Python layer and of the two getters
    tau1, M1, C1 = _id(world, st[:1], a[:1])
    assert torch.equal(tau1[0], tau[0]) and torch.equal(M1[0], M[0]) and torch.equal(C1[0], C[0])
    t1 = nimble.inverse_dynamics(world, _t(st[1]), _t(a[1]))
    assert tuple(t1.shape) == (n,) and torch.equal(t1, tau[1])
    assert torch.equal(nimble.mass_matrix(world, _t(st[1, :n])), M[1])
    assert torch.equal(nimble.mass_matrix(world, _t(st[:, :n])), M)
    assert torch.equal(nimble.coriolis_and_gravity(world, _t(st[1])), C[1])
    assert torch.equal(nimble.coriolis_and_gravity(world, _t(st)), C)
    print(name, {k: f"{v:.2e}" for k, v in e.items()})
    for k, v in e.items():
        assert v <= RTOL, (name, k, v)


# --- 2. round trip through the existing forward -------------------------------------
@pytest.mark.parametrize("name", FREE)
def test_round_trip_through_the_forward(name):
    """timestep(world, (q, v), tau) has v' = v + dt a; with wrenches, through
    the `_ext` forward given the same wrenches, in both frames."""
    world, st, a, ref, _ = _case(name)
    n = world.getNumDofs()
    want = st[:, n:] + ref.dt * a
    tau, _, _ = _id(world, st, a, extras=False)
    e = {"none": _rel(_forward(world, st, _np(tau))[:, n:], want)}
    W = _wrenches(world, B, seed=5)
    for frame in FRAMES:
        tw, _, _ = _id(world, st, a, bw=W, frame=frame, extras=False)
        assert not torch.equal(tw, tau)
        e[frame] = _rel(_forward(world, st, _np(tw), W, frame)[:, n:], want)
    print(name, {k: f"{v:.2e}" for k, v in e.items()})
    for k, v in e.items():
        assert v <= RTOL, (name, k, v)


# --- 3. the vector-Jacobian product --------------------------------------------------
def _first_dofs(world):
    """The first dof of each joint type of the model."""
    d = world.desc_arrays()
    ndof = {0: 0, 1: 1, 2: 1, 3: 6, 4: 3, 5: 3}
    seen = {}
    for b, t in enumerate(d["joint_type"]):
        if ndof[int(t)] > 0 and int(t) not in seen:
            seen[int(t)] = int(d["dof_offset"][b])
    return sorted(seen.values())


@pytest.mark.parametrize("name", FREE)
def test_vjp_against_the_analytic_reference(name):
    world, st, a, ref, _ = _case(name)
    n = world.getNumDofs()
    J = _analytic(name)
    rng = np.random.default_rng(9)
    gs_in = [rng.standard_normal((B, n)), rng.standard_normal((B, n))]
    for k in _first_dofs(world):
        e_k = np.zeros((B, n))
        e_k[:, k] = 1.0
        gs_in.append(e_k)
    worst = {"grad_state": 0.0, "grad_ddq": 0.0}
    for g in gs_in:
        gs, ga, _ = _id_bwd(world, st, a, g)
        rgs = np.stack([np.concatenate([J[b][0].T @ g[b], J[b][1].T @ g[b]]) for b in range(B)])
        rga = np.stack([J[b][2].T @ g[b] for b in range(B)])
        worst["grad_state"] = max(worst["grad_state"], _rel(_np(gs), rgs))
        worst["grad_ddq"] = max(worst["grad_ddq"], _rel(_np(ga), rga))
    print(name, len(gs_in), "upstream gradients", {k: f"{v:.2e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= RTOL, (name, k, v)


# --- 4. wrenches ---------------------------------------------------------------------
@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("name", ["compound", "atlas_air"])
def test_wrenches(name, frame):
    """tau(W) = tau(0) - tau_ext with tau_ext in numpy from the Tw / Sw the
    shared forward caches at the same q; grad_wrench = -(body twists under g)
    in the frame of the input; grad_state against Richardson differences of
    that reference tau (both frames: tau_ext depends on q through the S_k
    either way, a body-frame wrench also moves with the body)."""
    world, st, a, ref, tau_ref = _case(name)
    n = world.getNumDofs()
    up = _tree(world)
    W = _wrenches(world, B, seed=5)
    zero = np.zeros((B, n))
    Tw, Sw = _forward_kin(world, st, zero)
    text = _tau_ext(up, Sw, _to_world(W, Tw, frame))
    tau, _, _ = _id(world, st, a, bw=W, frame=frame, extras=False)
    e = {"tau": _rel(_np(tau), tau_ref - text)}
    assert np.abs(text).max() > 1e-2 * np.abs(tau_ref).max()  # (the wrenches matter)
    g = np.random.default_rng(13).standard_normal((B, n))
    gs, ga, gw = _id_bwd(world, st, a, g, bw=W, frame=frame, want_gw=True)
    e["grad_wrench"] = _rel(_np(gw), -_to_frame(_body_twists(up, Sw, g), Tw, frame))
    # Richardson differences of the reference tau: the oracle part on the CPU,
    # tau_ext at every perturbed q from one shared forward launch
    H = invdyn_refs.H
    steps = []
    for h in (H / 2, H):
        for k in range(n):
            for sgn in (1.0, -1.0):
                sp = st.copy()
                sp[:, k] += sgn * h
                steps.append(sp)
    allst = np.concatenate(steps)  # [4 n B, 2n]
    Twp, Swp = _forward_kin(world, allst, np.zeros((allst.shape[0], n)))
    tep = _tau_ext(up, Swp, _to_world(np.tile(W, (4 * n, 1, 1)), Twp, frame)).reshape(2, n, 2, B, n)
    dte = [(tep[i, :, 0] - tep[i, :, 1]) / (2 * h) for i, h in enumerate((H / 2, H))]  # [k, B, n]
    dtext = (4.0 * dte[0] - dte[1]) / 3.0
    rgs = np.zeros((B, 2 * n))
    JR = _richardson(name)
    for b in range(B):
        dq, dv, _ = JR[b]
        dq = dq - dtext[:, b, :].T  # d(tau_ref - tau_ext)/dq
        rgs[b] = np.concatenate([dq.T @ g[b], dv.T @ g[b]])
    e["grad_state"] = _rel(_np(gs), rgs)
    gs0, ga0, _ = _id_bwd(world, st, a, g)
    assert torch.equal(ga, ga0)                          # M g does not see the wrench
    assert torch.equal(gs[:, n:], gs0[:, n:])            # nor does dC/dv
    assert np.abs(_np(gs - gs0)[:, :n]).max() > 1e-6 * np.abs(rgs).max()
    print(name, frame, {k: f"{v:.2e}" for k, v in e.items()})
    for k, v in e.items():
        assert v <= RTOL, (name, frame, k, v)


# --- 5. per-world inertia --------------------------------------------------------------
@pytest.mark.parametrize("name", ["cartpole", "atlas_air"])
def test_per_world_inertia(name):
    """B = 6, world b with parameter set b % 3: tau against an oracle built per
    set; and the model's own values as rows give the bits of passing none."""
    world, st = _states(name, 6)
    n = world.getNumDofs()
    a = invdyn_refs.accelerations((6, n), seed=5)
    g = np.random.default_rng(3).standard_normal((6, n))
    sets = PW.param_sets(world)
    assert all(PW.positive_definite(P) for P in sets)
    bi = PW.batch_params(world, 6)
    tau, M, C = _id(world, st, a, bi=bi)
    worst = {"tau": 0.0, "mass_matrix": 0.0, "bias": 0.0}
    try:
        for k in range(PW.K):
            rows = [b for b in range(6) if b % PW.K == k]
            PW.set_world_params(world, sets[k])
            ref = invdyn_refs.Ref(world)
            worst["tau"] = max(worst["tau"], _rel(_np(tau)[rows], ref.tau_batch(st[rows], a[rows])))
            for b in rows:
                worst["mass_matrix"] = max(worst["mass_matrix"], _rel(_np(M)[b], ref.o.mass_matrix(st[b, :n])))
                worst["bias"] = max(worst["bias"], _rel(_np(C)[b], ref.o.coriolis_gravity(st[b, :n], st[b, n:])))
    finally:
        PW.set_world_params(world, sets[0])
    # (the sets matter: world 1, set 1, is far from the model's own answer)
    assert _rel(_np(tau)[1:2], _np(_id(world, st, a, extras=False)[0])[1:2]) > 1e-3
    own =np.tile(PW.base_params(world)[None], (6, 1, 1))
    for got, want in zip(_id(world, st, a, bi=own) + _id_bwd(world, st, a, g, bi=own)[:2],
                         _id(world, st, a) + _id_bwd(world, st, a, g)[:2]):
        assert torch.equal(got, want)
    print(name, {k: f"{v:.2e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= RTOL, (name, k, v)


# --- 6. autograd -------------------------------------------------------------------------
def test_autograd_equals_the_c_abi():
    """inverse_dynamics 2-D, 1-D and with CPU tensors: its gradients are the
    C-ABI outputs; mass 1-D / 2-D reach the kernels as per-world rows; the
    world is left as it was."""
    world, st, a, ref, _ = _case("compound")
    n = world.getNumDofs()
    nbw = world.getNumBodyNodes()
    assert world.native().nb > nbw  # (chain frames: world order != device order)
    rng = np.random.default_rng(17)
    Ww = rng.standard_normal((B, nbw, 6))
    g = rng.standard_normal((B, n))
    before = (world.getState().copy(), world.getControlForces().copy(), world._version)
    for frame in FRAMES:
        Wd = _np(world._scatter_wrench(torch.tensor(Ww)))
        tau_c, _, _ = _id(world, st, a, bw=Wd, frame=frame, extras=False)
        gs_c, ga_c, gw_c = _id_bwd(world, st, a, g, bw=Wd, frame=frame, want_gw=True)
        gw_c = world._gather_wrench(gw_c)
        for mode in ("2d", "1d", "cpu"):
            dev = "cpu" if mode == "cpu" else D
            rows = [1] if mode == "1d" else list(range(B))
            mk = lambda x: torch.tensor(x[1] if mode == "1d" else x, dtype=torch.float64, device=dev,  # noqa: E731
                                        requires_grad=True)
            ts, ta, tw = mk(st), mk(a), mk(Ww)
            tau = nimble.inverse_dynamics(world, ts, ta, body_wrench=tw, wrench_frame=frame)
            assert tau.device.type == ("cpu" if mode == "cpu" else "cuda")
            tau.backward(torch.tensor(g[1] if mode == "1d" else g, device=dev))
            pick = (lambda t: t[1]) if mode == "1d" else (lambda t: t)
            for got, want in ((tau.detach(), tau_c), (ts.grad, gs_c), (ta.grad, ga_c), (tw.grad, gw_c)):
                assert got.device.type == ("cpu" if mode == "cpu" else "cuda")
                assert torch.equal(got.to(D), pick(want)), (frame, mode, rows)
    after = (world.getState(), world.getControlForces(), world._version)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2]
    # mass: 2-D rows, and a 1-D vector for every world
    aw, ast = _states("atlas_air", B)
    for i in (2, 7):
        aw.tuneMass(aw.getSkeleton(0).getBodyNode(i), "INERTIA_MASS")
    m0 = aw.getMasses().copy()
    an = aw.getNumDofs()
    aa = invdyn_refs.accelerations((B, an), seed=5)
    m2 = torch.tensor(np.stack([m0 * s for s in (0.7, 1.0, 1.6)]), device=D)
    want, _, _ = _id(aw, ast, aa, bi=_np(aw._batched_inertia(m2)), extras=False)
    got = nimble.inverse_dynamics(aw, _t(ast), _t(aa), mass=m2)
    assert torch.equal(got, want) and not torch.equal(got[0], _id(aw, ast, aa, extras=False)[0][0])
    one = nimble.inverse_dynamics(aw, _t(ast), _t(aa), mass=m2[0])
    assert torch.equal(one[0], want[0]) and np.array_equal(aw.getMasses(), m0)
    with pytest.raises(ValueError, match="not differentiable"):
        nimble.inverse_dynamics(aw, _t(ast), _t(aa), mass=m2.clone().requires_grad_(True))


@pytest.mark.parametrize("name", ["cartpole", "atlas_air"])
def test_timestep_of_inverse_dynamics_has_unit_slope(name):
    """d/da of timestep(world, s, inverse_dynamics(world, s, a))[:, n:].sum()
    is dt in every element: v' = v + dt a through both layers' backward."""
    world, st, a, ref, _ = _case(name)
    n = world.getNumDofs()
    ts = _t(st)
    ta = _t(a).requires_grad_(True)
    nxt = nimble.timestep(world, ts, nimble.inverse_dynamics(world, ts, ta))
    assert _rel(_np(nxt.detach())[:, n:], st[:, n:] + ref.dt * a) <= RTOL
    nxt[:, n:].sum().backward()
    err = _rel(_np(ta.grad), np.full((B, n), ref.dt))
    print(name, f"{err:.2e}")
    assert err <= RTOL, (name, err)


def test_world_getters():
    world, st, a, ref, _ = _case("atlas_air")
    n = world.getNumDofs()
    before = world.getState().copy()
    try:
        world.setState(st[2])
        M, C = world.getMassMatrix(), world.getCoriolisAndGravityForces()
        assert isinstance(M, np.ndarray) and M.shape == (n, n) and C.shape == (n,)
        assert np.array_equal(M, _np(nimble.mass_matrix(world, _t(st[:, :n])))[2])
        assert np.array_equal(C, _np(nimble.coriolis_and_gravity(world, _t(st)))[2])
        assert np.array_equal(M, M.T)
        assert np.array_equal(world.getState(), st[2])
    finally:
        world.setState(before)
