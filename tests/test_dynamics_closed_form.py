"""Independent pins of the oracle's forward dynamics (CPU, no GPU).

The reference holds no dynamics golden outputs (its dynamics tests compare
Skeleton quantities with each other or with finite differences), so these
tests check the oracle -- which the GPU path is compared with -- against
closed forms derived by hand, not against its own identities:

* the cartpole's mass matrix, Coriolis + gravity and accelerations from the
  Lagrangian of the model python/nimblephysics_examples/cartpole.py builds
  (cart mass 1 on a prismatic x rail, pole mass 1 with I_zz = 1 whose COM sits
  l = 0.5 above the revolute joint);
* a free rigid body (FreeJoint, dart/dynamics/FreeJoint.cpp, generalized
  velocity = body-frame spatial velocity [w; v]) against the Newton-Euler
  equations: I dw = -w x I w, m (dv + w x v) = m R^T g;
* a rollout of the undamped cartpole against the same closed form integrated
  with the reference's update rules (World.cpp:221 integrateVelocities then
  integratePositions with the pre-step velocity by default, or the post-step
  one for sequential updates), and the energy of the sequential (symplectic
  Euler) rollout staying within its O(dt) band;
* the URDF loader's masses, COMs, inertias and joint frames of the bench Atlas
  (data/sdf/atlas/atlas_v3_box_colliders.urdf) against the URDF text, parsed
  here independently (the URDF is stored under tests/golden/reference_models).
"""
import json
import math
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import models
from nimblephysics_amd import dynamics as D
import nimblephysics_amd as nimble
from oracle import oracle as O

REF_ATLAS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_models", "data", "sdf",
                         "atlas", "atlas_v3_box_colliders.urdf")
G = 9.81


def _cartpole_closed_form(q, v):
    """M, C + g for cart (x, mass mc) + pole (theta, mass mp, I_zz, COM at
    l along the pole): p_com = (x - l sin th, l cos th)."""
    mc, mp, Izz, l = 1.0, 1.0, 1.0, 0.5
    x, th = q
    xd, thd = v
    M = np.array([[mc + mp, -mp * l * math.cos(th)],
                  [-mp * l * math.cos(th), Izz + mp * l * l]])
    Cg = np.array([mp * l * math.sin(th) * thd * thd, -mp * G * l * math.sin(th)])
    return M, Cg


def test_cartpole_mass_matrix_and_bias_closed_form(oracle_built):
    w = models.cartpole_world()
    o = O.OracleWorld(w)
    rng = np.random.default_rng(0)
    for _ in range(20):
        q = rng.uniform(-3, 3, 2)
        v = rng.uniform(-4, 4, 2)
        tau = rng.uniform(-5, 5, 2)
        M, Cg = _cartpole_closed_form(q, v)
        assert np.abs(o.mass_matrix(q) - M).max() < 1e-12
        assert np.abs(o.coriolis_gravity(q, v) - Cg).max() < 1e-12
        ddq = np.linalg.solve(M, tau - Cg)
        assert np.abs(o.forward_dynamics(q, v, tau) - ddq).max() < 1e-11 * max(1.0, np.abs(ddq).max())


def _free_body_world(mass, I, com, gravity):
    w = nimble.World()
    w.setGravity(gravity)
    sk = D.Skeleton("rigid")
    _, b = sk.createFreeJointAndBodyNodePair()
    b.setMass(mass)
    b.setMomentOfInertia(*I)
    b.setLocalCOM(com)
    w.addSkeleton(sk)
    return w


def _exp_so3(r):
    th = np.linalg.norm(r)
    K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / (th * th) * K @ K


@pytest.mark.parametrize("gravity", [(0.0, 0.0, 0.0), (0.0, -9.81, 0.0)])
def test_free_rigid_body_newton_euler(oracle_built, gravity):
    """Gyroscopic term and gravity in the body frame of a FreeJoint body with
    its COM at the body origin and a full (non-diagonal) inertia tensor."""
    Ixx, Iyy, Izz, Ixy, Ixz, Iyz = 0.3, 0.5, 0.7, 0.02, -0.03, 0.04
    m = 2.5
    w = _free_body_world(m, (Ixx, Iyy, Izz, Ixy, Ixz, Iyz), [0, 0, 0], gravity)
    I = np.array([[Ixx, Ixy, Ixz], [Ixy, Iyy, Iyz], [Ixz, Iyz, Izz]])
    o = O.OracleWorld(w)
    g = np.asarray(gravity)
    rng = np.random.default_rng(1)
    for _ in range(10):
        q = np.concatenate([rng.uniform(-1, 1, 3), rng.uniform(-2, 2, 3)])
        om, vl = rng.uniform(-3, 3, 3), rng.uniform(-2, 2, 3)
        v = np.concatenate([om, vl])
        R = _exp_so3(q[:3])
        # the oracle's own body rotation agrees with the exponential map
        assert np.abs(o.body_transforms(q)[0][:, :3] - R).max() < 1e-12
        dw = np.linalg.solve(I, -np.cross(om, I @ om))
        dv = -np.cross(om, vl) + R.T @ g
        ddq = o.forward_dynamics(q, v, np.zeros(6))
        assert np.abs(ddq - np.concatenate([dw, dv])).max() < 1e-11, (ddq, dw, dv)


def test_free_rigid_body_offset_com_momentum(oracle_built):
    """COM away from the body origin: the body-frame Newton-Euler equations
    about the origin, M [dw; dv] + [w x (I_o w) + m c x (w x v); m w x (v + w x c)] = 0
    with I_o = I_c - m [c]x^2 and M the 6x6 spatial inertia about the origin."""
    m, c = 1.7, np.array([0.1, -0.2, 0.05])
    Ic = np.diag([0.2, 0.3, 0.4])
    w = _free_body_world(m, (0.2, 0.3, 0.4), c, (0.0, 0.0, 0.0))
    o = O.OracleWorld(w)
    cx = np.array([[0, -c[2], c[1]], [c[2], 0, -c[0]], [-c[1], c[0], 0]])
    Io = Ic - m * cx @ cx
    Msp = np.block([[Io, m * cx], [-m * cx, m * np.eye(3)]])
    rng = np.random.default_rng(2)
    for _ in range(10):
        q = np.concatenate([rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)])
        om, vl = rng.uniform(-2, 2, 3), rng.uniform(-2, 2, 3)
        # momentum about the body origin h = Msp [w; v]; body-frame rate
        # equations dh/dt + [w x h_ang + v x h_lin; w x h_lin] = 0
        h = Msp @ np.concatenate([om, vl])
        bias = np.concatenate([np.cross(om, h[:3]) + np.cross(vl, h[3:]), np.cross(om, h[3:])])
        ddq_ref = np.linalg.solve(Msp, -bias)
        assert np.abs(o.mass_matrix(q) - Msp).max() < 1e-12
        ddq = o.forward_dynamics(q, np.concatenate([om, vl]), np.zeros(6))
        assert np.abs(ddq - ddq_ref).max() < 1e-11


@pytest.mark.parametrize("sequential", [False, True])
def test_cartpole_rollout_closed_form(oracle_built, sequential):
    """200 steps of the undamped, unforced cartpole: the oracle's trajectory
    equals the closed-form dynamics under the reference's update order."""
    w = models.cartpole_world()
    w.setParallelVelocityAndPositionUpdates(not sequential)
    dt = w.getTimeStep()
    st = np.array([[0.1, 0.8, 0.0, 0.3]])
    o = O.OracleWorld(w)
    q, v = st[0, :2].copy(), st[0, 2:].copy()
    x = st.copy()
    energies = []
    for _ in range(200):
        x = o.forward(x, np.zeros((1, 2)))
        M, Cg = _cartpole_closed_form(q, v)
        a = np.linalg.solve(M, -Cg)
        v1 = v + dt * a
        q = q + dt * (v1 if sequential else v)
        v = v1
        assert np.abs(x[0] - np.concatenate([q, v])).max() < 1e-9
        M1, _ = _cartpole_closed_form(q, v)
        energies.append(0.5 * v @ M1 @ v + 1.0 * G * 0.5 * math.cos(q[1]))
    if sequential:
        # symplectic Euler: the energy oscillates in an O(dt) band, no drift
        e = np.array(energies)
        assert e.max() - e.min() < 20 * dt * abs(e).max()


def _rpy(r, p, y):
    cr, sr, cp, sp, cy, sy = math.cos(r), math.sin(r), math.cos(p), math.sin(p), math.cos(y), math.sin(y)
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _nums(s, default="0 0 0"):
    return np.array([float(t) for t in (s or default).split()])


def test_atlas_asset_matches_urdf_text():
    """Masses, COMs, inertia tensors, joint origins and axes of the bench
    Atlas asset (what the GPU box loads) against the URDF's own numbers."""
    root = ET.parse(REF_ATLAS).getroot()
    links = {l.get("name"): l for l in root.findall("link")}
    joints = {j.find("child").get("link"): j for j in root.findall("joint")}
    with open(os.path.join(os.path.dirname(nimble.__file__), "assets", "atlas.json")) as fh:
        asset = json.load(fh)
    names = [b["name"] for b in asset["bodies"]]
    assert sorted(names) == sorted(links)
    checked = 0
    for bd in asset["bodies"]:
        ln = links[bd["name"]]
        inert = ln.find("inertial")
        if inert is not None:
            assert bd["mass"] == float(inert.find("mass").get("value"))
            org = inert.find("origin")
            xyz = _nums(org.get("xyz") if org is not None else None)
            rpy = _nums(org.get("rpy") if org is not None else None)
            assert np.allclose(bd["com"], xyz, rtol=0, atol=1e-15)
            e = inert.find("inertia")
            g = lambda k: float(e.get(k, 0.0))
            J = np.array([[g("ixx"), g("ixy"), g("ixz")], [g("ixy"), g("iyy"), g("iyz")],
                          [g("ixz"), g("iyz"), g("izz")]])
            R = _rpy(*rpy)
            J = R @ J @ R.T
            Ixx, Iyy, Izz, Ixy, Ixz, Iyz = bd["moment"]
            assert np.allclose([Ixx, Iyy, Izz, Ixy, Ixz, Iyz],
                               [J[0, 0], J[1, 1], J[2, 2], J[0, 1], J[0, 2], J[1, 2]], rtol=1e-14, atol=1e-15)
        if bd["name"] in joints:
            j = joints[bd["name"]]
            assert bd["joint"]["name"] == j.get("name")
            parent = j.find("parent").get("link")
            assert names[bd["parent"]] == parent
            org = j.find("origin")
            T = np.array(bd["joint"]["T_parent"])
            assert np.allclose(T[:3, 3], _nums(org.get("xyz")), rtol=0, atol=1e-15)
            assert np.allclose(T[:3, :3], _rpy(*_nums(org.get("rpy"))), rtol=0, atol=1e-14)
            ax = j.find("axis")
            assert np.allclose(bd["joint"]["axis"], _nums(ax.get("xyz") if ax is not None else None, "1 0 0"))
            kind = {"revolute": D.JOINT_REVOLUTE, "continuous": D.JOINT_REVOLUTE, "prismatic": D.JOINT_PRISMATIC,
                    "fixed": D.JOINT_WELD}[j.get("type")]
            assert bd["joint"]["type"] == kind
            checked += 1
        else:
            assert bd["parent"] == -1 and bd["joint"]["type"] == D.JOINT_FREE
    assert checked == len(links) - 1
