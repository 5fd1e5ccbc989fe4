"""External body wrenches (body_wrench [B, nb, 6], the `_ext` entry points)
on the GPU.

The oracle has no external wrench.  The reference of every check is the
shared-model path, which the rest of the suite pins to the oracle, plus numpy
on the Sw (world-frame motion subspace columns) and Tw (body world transforms)
that path stores in the snapshot's dynamics cache: the generalized force of
the wrenches is  tau_ext[k] = Sw_k . sum_{b in subtree(body(k))} W_b  with W_b
the world-frame wrench of body b (a body-frame wrench is taken there with
Tw_b first), so a step with wrenches must be the shared-model step with
tau_ext added to the joint forces.

Results before this feature: FEATURE MISSING -- the `_ext` symbols, the
`body_wrench` keyword and the BodyNode setters do not exist, so every test
here fails on the parent commit.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import models
import per_world_params as PW
from nimblephysics_amd import _native, neural
from test_gpu_contact_parity import GRAD_FLOOR, RTOL, SN_M, SN_NC, SN_NU, SN_STATUS, _rel
from test_gpu_per_world_inertia import (MESH_WIDE_WORLD, OUTPUTS, _assert_rows_equal, _atlas_air, _atlas_contact,
                                        _atlas_mesh, _cartpole, _compound, _dyn_cache_doubles, _run)

pytestmark = pytest.mark.gpu

EXT_OUTPUTS = OUTPUTS + ("grad wrench", "wrench Jacobian")
FRAMES = ("world", "body")
SN_CFM, SN_PATH0, SN_PATH1 = 4, 6, 7  # the LCP's path flags in the snapshot header (as __graft_entry__.smoke)


def _ball():
    w = models.ball_world()
    return w, models.ball_states(4, seed=2)


MODELS = {"cartpole": _cartpole, "atlas_air": _atlas_air, "atlas_contact": _atlas_contact, "compound": _compound,
          "ball": _ball, "atlas_mesh": _atlas_mesh}


# --- numpy reference on the dynamics cache --------------------------------------
def _tree(world):
    """(dof -> body, anc[b]: the bodies on the path from b to its root, b
    included) of the device model, from the world's description."""
    d = world.desc_arrays()
    nb = int(d["num_bodies"])
    ndof = [{0: 0, 1: 1, 2: 1, 3: 6, 4: 3, 5: 3}[int(t)] for t in d["joint_type"]]
    dof_body = np.zeros(int(d["num_dofs"]), dtype=np.int64)
    for b in range(nb):
        dof_body[int(d["dof_offset"][b]):int(d["dof_offset"][b]) + ndof[b]] = b
    anc = []
    for b in range(nb):
        s, p = {b}, int(d["parent"][b])
        while p >= 0:
            s.add(p)
            p = int(d["parent"][p])
        anc.append(s)
    # up[k, b] = 1 when body(k) is b or an ancestor of b (b in the subtree of dof k)
    up = np.array([[1.0 if dof_body[k] in anc[b] else 0.0 for b in range(nb)] for k in range(len(dof_body))])
    return up.reshape(len(dof_body), nb)


def _kin(dyn, n, nb):
    """Tw [B, nb, 3, 4] and Sw [B, n, 6] of a dynamics cache [B, ...]."""
    dyn = np.asarray(dyn)
    return dyn[:, :12 * nb].reshape(-1, nb, 3, 4), dyn[:, 12 * nb:12 * nb + 6 * n].reshape(-1, n, 6)


def _to_world(W, Tw, frame):
    """World-frame wrenches [B, nb, 6] of the input wrenches: as given, or
    dAdInvT(Tw, F) = [R t + p x (R f); R f]."""
    if frame == "world":
        return W
    R, p = Tw[..., :3], Tw[..., 3]
    rt = np.einsum("...ij,...j->...i", R, W[..., :3])
    rf = np.einsum("...ij,...j->...i", R, W[..., 3:])
    return np.concatenate([rt + np.cross(p, rf), rf], axis=-1)


def _to_frame(V, Tw, frame):
    """A world twist [..., nb, 6] in the wrench's frame: as it is, or
    Ad_{Tw^-1} V = [R^T w; R^T (v + w x p)]."""
    if frame == "world":
        return V
    R, p = Tw[..., :3], Tw[..., 3]
    u = V[..., 3:] + np.cross(V[..., :3], p)
    return np.concatenate([np.einsum("...ji,...j->...i", R, V[..., :3]), np.einsum("...ji,...j->...i", R, u)], axis=-1)


def _tau_ext(up, Sw, Ww):
    """tau_ext [B, n]: Sw_k . (sum of the world wrenches in dof k's subtree)."""
    G = np.einsum("kb,Bbi->Bki", up, Ww)
    return np.einsum("Bki,Bki->Bk", Sw, G)


def _body_twists(up, Sw, w):
    """[..., nb, 6]: sum over the dofs k on the path to body b of Sw_k w_k."""
    return np.einsum("kb,Bki,B...k->B...bi", up, Sw, w)


def _wrenches(world, B, seed):
    """Random wrenches on every device body, forces about m_b |g| and torques
    about m_b |g| x 0.1 m, so the wrench term is comparable to gravity's
    (massless chain frames and light bodies: as for 0.5 kg)."""
    d = world.desc_arrays()
    m = np.maximum(np.asarray(d["mass"], dtype=np.float64), 0.5) * np.linalg.norm(d["gravity"])
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((B, len(m), 6)) * m[None, :, None]
    W[:, :, :3] *= 0.1
    return W


# --- device runs ----------------------------------------------------------------------
def _run_ext(world, st, f, g, bw, frame, bi=None):
    """_run of the per-world file with body_wrench: forward, the three
    backward modes, both Jacobian modes through the `_ext` entry points, plus
    grad_wrench and the wrench Jacobian.  Returns EXT_OUTPUTS."""
    dev = world.native()
    d = torch.device("cuda:0")
    B = st.shape[0]
    ts, tf, tg = torch.tensor(st, device=d), torch.tensor(f, device=d), torch.tensor(g, device=d)
    tbi = None if bi is None else torch.tensor(bi, device=d)
    kw = {"body_inertia": tbi, "body_wrench": torch.tensor(bw, device=d), "wrench_frame": frame}
    cache = torch.zeros((B, dev.cache_doubles), dtype=torch.float64, device=d)
    cache[:, 0] = -1
    nxt = torch.empty_like(ts)
    snap = torch.zeros((B, dev.snapshot_doubles), dtype=torch.float64, device=d)
    stream = torch.cuda.current_stream().cuda_stream
    dev.forward(ts, tf, cache, nxt, snap, stream, **kw)
    gs, gf = torch.empty_like(ts), torch.empty_like(tf)
    gw = torch.full((B, dev.nb, 6), float("nan"), dtype=torch.float64, device=d)
    dev.backward(ts, tf, snap, tg, gs, gf, stream, grad_wrench=gw, **kw)
    gs1, gf1 = torch.empty_like(ts), torch.empty_like(tf)
    gm = torch.empty((B, dev.nb), dtype=torch.float64, device=d)
    dev.backward_masses(ts, tf, snap, tg, gs1, gf1, gm, stream, **kw)
    gs2, gf2 = torch.empty_like(ts), torch.empty_like(tf)
    gi = torch.empty((B, dev.nb, 10), dtype=torch.float64, device=d)
    dev.backward_inertia(ts, tf, snap, tg, gs2, gf2, gi, stream, **kw)
    J, F, WJ = dev.jacobians(ts, tf, snap, stream, wrench_jacobian=True, **kw)
    Js, Jf = dev.constraint_force_jacobians(ts, tf, snap, stream, **kw)
    torch.cuda.synchronize()
    assert torch.equal(gs, gs1) and torch.equal(gs, gs2) and torch.equal(gf, gf1) and torch.equal(gf, gf2)
    if dev.num_pairs > 0:
        fc = snap[:, _native.SN_FC:_native.SN_FC + _native.MAX_LCP].clone()
        header = snap[:, :SN_STATUS + 1].clone()
        path = torch.stack([snap[:, SN_CFM], (snap[:, SN_STATUS].to(torch.int64) & 8).to(torch.float64),
                            snap[:, SN_PATH0], snap[:, SN_PATH1]], dim=1).cpu().numpy()
    else:
        fc, header, path = snap[:, :0].clone(), snap[:, :8].clone(), np.zeros((B, 4))
    dyn = snap[:, dev.snapshot_doubles - _dyn_cache_doubles(dev.n, dev.nb):].clone()
    return (nxt, cache, header, fc, dyn, gs, gf, gm, gi, J, F, Js, Jf, gw, WJ), path


def _path_flags(world, st, f):
    """The LCP path flags (fallback CFM, reduced, and the two solver-path
    slots of the header) of a shared-model forward."""
    dev = world.native()
    d = torch.device("cuda:0")
    B = st.shape[0]
    if dev.num_pairs == 0:
        return np.zeros((B, 4))
    ts, tf = torch.tensor(st, device=d), torch.tensor(f, device=d)
    cache = torch.zeros((B, dev.cache_doubles), dtype=torch.float64, device=d)
    cache[:, 0] = -1
    nxt = torch.empty_like(ts)
    snap = torch.zeros((B, dev.snapshot_doubles), dtype=torch.float64, device=d)
    dev.forward(ts, tf, cache, nxt, snap, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return torch.stack([snap[:, SN_CFM], (snap[:, SN_STATUS].to(torch.int64) & 8).to(torch.float64),
                        snap[:, SN_PATH0], snap[:, SN_PATH1]], dim=1).cpu().numpy()


def _forward_kin(world, st, f):
    """Tw, Sw of a shared-model forward at `st` (only its dynamics cache is
    read; any batch size, in one launch)."""
    dev = world.native()
    d = torch.device("cuda:0")
    B = st.shape[0]
    ts, tf = torch.tensor(st, device=d), torch.tensor(f, device=d)
    cache = torch.zeros((B, dev.cache_doubles), dtype=torch.float64, device=d)
    cache[:, 0] = -1
    nxt = torch.empty_like(ts)
    snap = torch.zeros((B, dev.snapshot_doubles), dtype=torch.float64, device=d)
    dev.forward(ts, tf, cache, nxt, snap, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    dyn = snap[:, dev.snapshot_doubles - _dyn_cache_doubles(dev.n, dev.nb):].cpu().numpy()
    return _kin(dyn, dev.n, dev.nb)


@functools.lru_cache(maxsize=None)
def _base(name):
    """Model, states, upstream gradient, wrenches and run A (shared path,
    forces f), made once per model."""
    world, (st, f) = MODELS[name]()
    world.setStatusPolicy("record")
    g = np.random.default_rng(11).standard_normal(st.shape)
    A = _run(world, st, f, g)
    dev = world.native()
    Tw, Sw = _kin(A[4].cpu().numpy(), dev.n, dev.nb)
    W = _wrenches(world, st.shape[0], seed=5)
    return world, st, f, g, A, Tw, Sw, _tree(world), W


@functools.lru_cache(maxsize=None)
def _triple(name, frame):
    """Runs B (shared path, forces f + tau_ext) and C (`_ext` path, forces f,
    the wrenches) of one model and frame."""
    world, st, f, g, A, Tw, Sw, up, W = _base(name)
    tau = _tau_ext(up, Sw, _to_world(W, Tw, frame))
    Bm = _run(world, st, f + tau, g)
    pathB = _path_flags(world, st, f + tau)
    Cm, pathC = _run_ext(world, st, f, g, W, frame)
    return Bm, Cm, pathB, pathC, tau


def _np(t):
    return t.cpu().numpy()


# --- 1. zero wrench, same bits -----------------------------------------------------
@pytest.mark.parametrize("name", ["cartpole", "atlas_air", "atlas_contact", "compound", "atlas_mesh"])
def test_zero_wrench_same_bits(name):
    """An all-zero body_wrench through the `_ext` path (either frame) gives
    the bits of the existing entry points in every output of _run."""
    world, st, f, g, A, Tw, Sw, up, W = _base(name)
    B = st.shape[0]
    for frame in FRAMES:
        Z, _ = _run_ext(world, st, f, g, np.zeros_like(W), frame)
        _assert_rows_equal(f"{name} {frame}", Z[:len(OUTPUTS)], A, list(range(B)))
    if name == "atlas_mesh":
        m = dict(zip(OUTPUTS, A))["snapshot header"][:, SN_M].tolist()
        assert m[MESH_WIDE_WORLD] > 64 and max(m[:MESH_WIDE_WORLD]) <= 64, m


def test_null_wrench_is_the_existing_path():
    """nimble_forward_ext / nimble_backward_ext with a NULL body_wrench are
    the existing entry points."""
    world, st, f, g, A, Tw, Sw, up, W = _base("atlas_contact")
    dev = world.native()
    d = torch.device("cuda:0")
    B = st.shape[0]
    ts, tf, tg = torch.tensor(st, device=d), torch.tensor(f, device=d), torch.tensor(g, device=d)
    cache = torch.zeros((B, dev.cache_doubles), dtype=torch.float64, device=d)
    cache[:, 0] = -1
    nxt = torch.empty_like(ts)
    snap = torch.zeros((B, dev.snapshot_doubles), dtype=torch.float64, device=d)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p, null = _native._ptr, C.c_void_p(0)
    L = _native.lib()
    _native._check(L.nimble_forward_ext(dev.h, B, p(ts), p(tf), p(cache), p(nxt), p(snap), null, null, 1, stream))
    gs, gf = torch.empty_like(ts), torch.empty_like(tf)
    _native._check(L.nimble_backward_ext(dev.h, B, p(ts), p(tf), p(snap), p(tg), p(gs), p(gf), null, null, 0, null,
                                         stream))
    torch.cuda.synchronize()
    ref = dict(zip(OUTPUTS, A))
    assert torch.equal(nxt, ref["next state"]) and torch.equal(cache, ref["LCP cache"])
    assert torch.equal(gs, ref["grad state"]) and torch.equal(gf, ref["grad forces"])


# --- 2. equivalent joint torque ------------------------------------------------------
def _comparable(name, pathB, pathC):
    """Worlds whose runs B and C took the same LCP path; at most 1 of the 8
    ground worlds and none of the mesh worlds may differ."""
    same = (pathB == pathC).all(axis=1)
    allowed = {"atlas_contact": 1}.get(name, 0)
    assert (~same).sum() <= allowed, (name, pathB.tolist(), pathC.tolist())
    return np.nonzero(same)[0]


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_equivalent_joint_torque(name, frame):
    """Run C (wrenches) against run B (their generalized force added to the
    joint forces): next state, LCP size, f_c, gradients, force Jacobian; the
    bars of test_gpu_contact_parity."""
    world, st, f, g, A, Tw, Sw, up, W = _base(name)
    Bm, Cm, pathB, pathC, tau = _triple(name, frame)
    n = world.getNumDofs()
    rows = _comparable(name, pathB, pathC)
    b = {k: _np(v)[rows] for k, v in zip(OUTPUTS, Bm)}
    c = {k: _np(v)[rows] for k, v in zip(EXT_OUTPUTS, Cm)}
    a = {k: _np(v)[rows] for k, v in zip(OUTPUTS, A)}
    if name == "atlas_contact":
        m = _np(Cm[2])[:, SN_M]
        assert (m >= 12).any() and (m < 12).any(), m.tolist()  # both backward pool placements
    if name == "atlas_mesh":
        m = _np(Cm[2])[:, SN_M].tolist()
        assert m[MESH_WIDE_WORLD] > 64 and max(m[:MESH_WIDE_WORLD]) <= 64, m  # wide forward and backward
    errs = {"next q": _rel(c["next state"][:, :n], b["next state"][:, :n]),
            "next v": _rel(c["next state"][:, n:], b["next state"][:, n:]),
            "f_c": _rel(c["f_c"], b["f_c"]),
            "grad forces": _rel(c["grad forces"], b["grad forces"], GRAD_FLOOR),
            "grad v": _rel(c["grad state"][:, n:], b["grad state"][:, n:], GRAD_FLOOR),
            "grad masses": _rel(c["grad masses"], b["grad masses"], GRAD_FLOOR),
            "grad inertia": _rel(c["grad inertia"], b["grad inertia"], GRAD_FLOOR),
            "force Jacobian": _rel(c["force Jacobian"], b["force Jacobian"], GRAD_FLOOR)}
    print(name, frame, "rows", rows.tolist(), {k: f"{v:.2e}" for k, v in errs.items()})
    assert np.array_equal(c["LCP cache"][:, 0], b["LCP cache"][:, 0])
    if world.native().num_pairs > 0:
        for k in (SN_M, SN_NC, SN_NU):
            assert np.array_equal(c["snapshot header"][:, k], b["snapshot header"][:, k]), k
    for k, v in errs.items():
        assert v < RTOL, (k, v)
    # the wrench does something: C is not A
    assert _rel(c["next state"][:, n:], a["next state"][:, n:]) > 1e-3


# --- 3. grad_wrench and the wrench Jacobian -----------------------------------------
@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_grad_wrench_and_jacobian(name, frame):
    """grad_wrench_b = sum over the dofs k on b's path of Sw_k (F^T g)_k with F
    run B's (unclipped) force Jacobian, taken to body axes for the body
    frame; wrench_jacobian row r is the same with upstream e_r."""
    world, st, f, g, A, Tw, Sw, up, W = _base(name)
    Bm, Cm, pathB, pathC, tau = _triple(name, frame)
    rows = _comparable(name, pathB, pathC)
    F = _np(Bm[10])                                   # [B, 2n, n]
    gt = np.einsum("Brk,Br->Bk", F, g)
    ref = _to_frame(_body_twists(up, Sw, gt), Tw, frame)
    refJ = _to_frame(_body_twists(up, Sw, F), Tw[:, None], frame)
    gw, WJ = _np(Cm[13]), _np(Cm[14])
    e1, e2 = _rel(gw[rows], ref[rows], GRAD_FLOOR), _rel(WJ[rows], refJ[rows], GRAD_FLOOR)
    e3 = _rel(np.einsum("Brbi,Br->Bbi", WJ, g)[rows], gw[rows], GRAD_FLOOR)
    print(name, frame, f"grad_wrench {e1:.2e} wrench_jacobian {e2:.2e} rows.g vs grad_wrench {e3:.2e}")
    assert e1 < RTOL and e2 < RTOL and e3 < RTOL, (e1, e2, e3)


# --- 4. position gradient ---------------------------------------------------------------
def _steps(q):
    """Central-difference steps relative to the coordinate (test_gpu_mass
    _mass_parity: 1e-5 of the value; coordinates near zero as 0.1)."""
    return 1e-5 * np.maximum(np.abs(q), 0.1)


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("name", ["atlas_air", "atlas_contact", "compound", "ball"])
def test_position_gradient(name, frame):
    """grad_q(C) - grad_q(B) against the central difference over q of
    tau_ext(q) . (F^T g), tau_ext(q +- e) in numpy from the Sw / Tw of
    shared-path forwards at the perturbed states (world wrench held fixed for
    the world frame, transformed with the perturbed Tw for the body frame)."""
    world, st, f, g, A, Tw, Sw, up, W = _base(name)
    Bm, Cm, pathB, pathC, tau = _triple(name, frame)
    rows = _comparable(name, pathB, pathC)
    n = world.getNumDofs()
    B = st.shape[0]
    gt = np.einsum("Brk,Br->Bk", _np(Bm[10]), g)      # F^T g, unclipped
    e = _steps(st[:, :n])                             # [B, n]
    pert = np.repeat(st[:, None, None, :], n, axis=1).repeat(2, axis=2)  # [B, n, 2, 2n]
    for k in range(n):
        pert[:, k, 0, k] += e[:, k]
        pert[:, k, 1, k] -= e[:, k]
    Twp, Swp = _forward_kin(world, pert.reshape(-1, 2 * n), np.repeat(f, 2 * n, axis=0))
    Wrep = np.repeat(W, 2 * n, axis=0)
    taup = _tau_ext(up, Swp, _to_world(Wrep, Twp, frame)).reshape(B, n, 2, n)
    Lpm = np.einsum("Bksj,Bj->Bks", taup, gt)
    cd = (Lpm[:, :, 0] - Lpm[:, :, 1]) / (2 * e)
    got = _np(Cm[5])[:, :n] - _np(Bm[5])[:, :n]
    noise = 1e-14 * np.abs(Lpm).max() / e
    err = np.abs(got - cd)[rows]
    bound = (1e-6 * np.abs(cd[rows]).max() + noise)[rows]
    print(name, frame, f"max err {err.max():.3e} of {np.abs(cd[rows]).max():.3e}, noise {noise.max():.1e}")
    assert np.abs(cd[rows]).max() > 0
    assert (err <= bound).all(), (err.max(axis=0), np.abs(cd).max(axis=0))


# --- 5. end to end, no contact -------------------------------------------------------------
def _ext_forward(world, st, f, bw, frame):
    dev = world.native()
    d = torch.device("cuda:0")
    B = st.shape[0]
    ts, tf = torch.tensor(st, device=d), torch.tensor(f, device=d)
    cache = torch.zeros((B, dev.cache_doubles), dtype=torch.float64, device=d)
    cache[:, 0] = -1
    nxt = torch.empty_like(ts)
    snap = torch.zeros((B, dev.snapshot_doubles), dtype=torch.float64, device=d)
    dev.forward(ts, tf, cache, nxt, snap, torch.cuda.current_stream().cuda_stream,
                body_wrench=torch.tensor(bw, device=d), wrench_frame=frame)
    torch.cuda.synchronize()
    return _np(nxt)


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("name", ["cartpole", "atlas_air"])
def test_end_to_end_central_differences(name, frame):
    """grad_state and grad_wrench of the `_ext` path against central
    differences of the `_ext` forward itself, loss g . next_state."""
    world, st, f, g, A, Tw, Sw, up, W = _base(name)
    Bm, Cm, pathB, pathC, tau = _triple(name, frame)
    B, S = st.shape
    nb = W.shape[1]
    P = S + 6 * nb
    x = np.concatenate([st, W.reshape(B, -1)], axis=1)          # [B, P]
    e = _steps(x)
    pert = np.repeat(x[:, None, None, :], P, axis=1).repeat(2, axis=2)
    for k in range(P):
        pert[:, k, 0, k] += e[:, k]
        pert[:, k, 1, k] -= e[:, k]
    pert = pert.reshape(-1, P)
    nxt = _ext_forward(world, np.ascontiguousarray(pert[:, :S]), np.repeat(f, 2 * P, axis=0),
                       np.ascontiguousarray(pert[:, S:]).reshape(-1, nb, 6), frame)
    L = np.einsum("Bksj,Bj->Bks", nxt.reshape(B, P, 2, S), g)
    cd = (L[:, :, 0] - L[:, :, 1]) / (2 * e)
    got = np.concatenate([_np(Cm[5]), _np(Cm[13]).reshape(B, -1)], axis=1)
    noise = 1e-14 * np.abs(L).max() / e
    for label, sl in (("grad_state", slice(0, S)), ("grad_wrench", slice(S, P))):
        err = np.abs(got - cd)[:, sl]
        bound = 1e-6 * np.abs(cd[:, sl]).max() + noise[:, sl]
        print(name, frame, label, f"max err {err.max():.3e} of {np.abs(cd[:, sl]).max():.3e}")
        assert (err <= bound).all(), (label, err.max(axis=0), np.abs(cd[:, sl]).max(axis=0))


# --- 6. closed form ---------------------------------------------------------------------------
def test_closed_form_free_box():
    """A free box of mass m in the air, at rest, not rotated.  Its COM is at
    its frame origin (asserted), so a body-frame force F at the body origin
    for one step changes the translational velocity by dt F / m and a
    world-frame pure force through the COM (moment p x F about the world
    origin) leaves the angular velocity as it was; both to 1e-12 of dt |F| / m."""
    world = models.box_world(ground=False)
    body = world.getSkeleton(0).getBodyNode(0)
    assert np.array_equal(body.getLocalCOM(), np.zeros(3))
    m, dt = body.getMass(), world.getTimeStep()
    st = np.zeros((1, 12))
    st[0, 3:6] = [0.3, 0.5, -0.2]
    f = np.zeros((1, 6))
    F = np.array([1.5, -2.0, 0.7])
    zero = np.zeros((1, 1, 6))
    base = _ext_forward(world, st, f, zero, "body")
    Wb = zero.copy()
    Wb[0, 0, 3:] = F
    out = _ext_forward(world, st, f, Wb, "body")
    dv = out[0, 6:] - base[0, 6:]
    scale = dt * np.linalg.norm(F) / m
    assert np.abs(dv[3:] - dt * F / m).max() <= 1e-12 * scale, dv
    assert np.abs(dv[:3]).max() <= 1e-12 * scale, dv
    Ww = zero.copy()
    Ww[0, 0, :3] = np.cross(st[0, 3:6], F)
    Ww[0, 0, 3:] = F
    out = _ext_forward(world, st, f, Ww, "world")
    dv = out[0, 6:] - base[0, 6:]
    assert np.abs(dv[:3]).max() <= 1e-12 * scale, dv
    assert np.abs(dv[3:] - dt * F / m).max() <= 1e-12 * scale, dv


# --- 7. with per-world inertia -----------------------------------------------------------------
def test_with_per_world_inertia():
    """Atlas on the ground, three parameter sets and a wrench: world by world
    the bits of the `_ext` path on a device model built with that set."""
    world, st, f, g, A, Tw, Sw, up, W = _base("atlas_contact")
    B = st.shape[0]
    sets = PW.param_sets(world)
    per, _ = _run_ext(world, st, f, g, W, "body", bi=PW.batch_params(world, B))
    try:
        for k in (1, 2, 0):
            PW.set_world_params(world, sets[k])
            ref, _ = _run_ext(world, st, f, g, W, "body")
            sel = [b for b in range(B) if b % PW.K == k]
            for label, x, y in zip(EXT_OUTPUTS, per, ref):
                assert torch.equal(x[sel], y[sel]), (k, label)
    finally:
        PW.set_world_params(world, sets[0])
    assert not torch.equal(per[0][1], _triple("atlas_contact", "body")[1][0][1])  # (the sets change the step)


# --- 8. autograd and API ----------------------------------------------------------------------------
def test_timestep_two_dimensional_wrench():
    """timestep with a [B, nBodies, 6] wrench in the world's body order (the
    compound rig: device model with chain frames); body_wrench.grad is check
    3's, and the step is the `_ext` path's."""
    import nimblephysics_amd as nimble
    world, st, f, g, A, Tw, Sw, up, W = _base("compound")
    rows = world._wrench_device_rows()
    nbw = world.getNumBodyNodes()
    assert len(rows) == nbw < W.shape[1]
    d = torch.device("cuda:0")
    for frame in FRAMES:
        Ww = np.zeros_like(W)
        Ww[:, rows] = W[:, rows]                       # (chain frames take none through this API)
        Cm, _ = _run_ext(world, st, f, g, Ww, frame)
        ts = torch.tensor(st, device=d, requires_grad=True)
        tf = torch.tensor(f, device=d, requires_grad=True)
        tw = torch.tensor(np.ascontiguousarray(W[:, rows]), device=d, requires_grad=True)
        world._batch_state = None
        out = nimble.timestep(world, ts, tf, body_wrench=tw, wrench_frame=frame)
        out.backward(torch.tensor(g, device=d))
        assert tuple(tw.grad.shape) == (st.shape[0], nbw, 6)
        assert torch.equal(out.detach(), Cm[0]) and torch.equal(ts.grad, Cm[5]) and torch.equal(tf.grad, Cm[6])
        assert torch.equal(tw.grad, Cm[13][:, torch.as_tensor(rows, device=d)])
    with pytest.raises(ValueError):
        nimble.timestep(world, ts, tf, body_wrench=tw[:, :nbw - 1])
    with pytest.raises(ValueError):
        nimble.timestep(world, ts, tf, body_wrench=tw, wrench_frame="local")
    # with a 1-D and a 2-D mass
    world.tuneMass(world.getSkeleton(0).getBodyNode(1), "INERTIA_MASS")
    try:
        m0 = world.getMasses()
        for mass in (torch.tensor(m0, device=d, requires_grad=True),
                     torch.tensor(np.repeat(m0[None], st.shape[0], axis=0), device=d, requires_grad=True)):
            tw2 = tw.detach().clone().requires_grad_(True)
            world._batch_state = None
            out = nimble.timestep(world, ts.detach(), tf.detach(), mass, tw2, "body")
            out.backward(torch.tensor(g, device=d))
            assert torch.equal(tw2.grad, tw.grad) and mass.grad.shape == mass.shape
            assert bool((mass.grad != 0).any())
    finally:
        world._mass_tuned.clear()


def test_stored_wrench_one_world():
    """A 1-D state with the wrench stored through BodyNode.setExtWrench is the
    explicit argument's step; the stored wrench is cleared after the step and
    kept by forwardPass(idempotent=True); lossWrtBodyWrench and the wrench
    Jacobian come back in the world's body order."""
    import nimblephysics_amd as nimble
    world = models.compound_world()
    world.setStatusPolicy("record")
    st, f = models.compound_states(1, seed=4)
    bodies = world._world_bodies()
    W = _wrenches(world, 1, seed=9)[0, world._wrench_device_rows()]
    d = torch.device("cuda:0")
    ts, tf = torch.tensor(st[0], device=d), torch.tensor(f[0], device=d)
    world._batch_state = None
    ref = nimble.timestep(world, ts, tf, body_wrench=torch.tensor(W, device=d), wrench_frame="body")
    for b, w in zip(bodies, W):
        b.setExtWrench(w)
    assert np.array_equal(bodies[1].getExternalForceLocal(), W[1])
    world._batch_state = None
    out = nimble.timestep(world, ts, tf)
    assert torch.equal(out, ref)
    assert all(not b.getExternalForceLocal().any() for b in bodies)  # World.cpp:300
    world._batch_state = None
    plain = nimble.timestep(world, ts, tf)
    assert not torch.equal(plain, ref)
    # forwardPass(world): picked up, kept under idempotent, cleared otherwise
    n = world.getNumDofs()
    for idem in (True, False):
        world.setState(st[0])
        world.setControlForces(f[0])
        for b, w in zip(bodies, W):
            b.setExtWrench(w)
        world._batch_state = None
        snap = neural.forwardPass(world, idempotent=idem)
        assert np.array_equal(np.concatenate([snap.getPostStepPosition(), snap.getPostStepVelocity()]), ref.cpu().numpy())
        assert any(b.getExternalForceLocal().any() for b in bodies) == idem
    g = np.random.default_rng(2).standard_normal(2 * n)
    bp = snap.backpropState(world, g)
    WJ = snap.getBodyWrenchJacobian(world)
    assert bp.lossWrtBodyWrench.shape == (len(bodies), 6) and WJ.shape == (2 * n, len(bodies), 6)
    assert _rel(np.einsum("rbi,r->bi", WJ, g), bp.lossWrtBodyWrench, GRAD_FLOOR) < RTOL
    assert np.abs(bp.lossWrtBodyWrench).max() > 0
    # World.step: the same step, wrenches cleared
    world.setState(st[0])
    world.setControlForces(f[0])
    for b, w in zip(bodies, W):
        b.addExtForce(w[3:], [0, 0, 0], True, True)
        b.addExtTorque(w[:3], True)
    world._batch_state = None
    world.step()
    assert np.array_equal(world.getState(), ref.cpu().numpy())
    assert all(not b.getExternalForceLocal().any() for b in bodies)
