"""Shared pieces of the contact inverse-dynamics tests (test infrastructure):
the 12-dof biped rig, and the numpy restatement of the reference's formulas
(Skeleton::getMultipleContactInverseDynamics, dart/dynamics/Skeleton.cpp:9578)
-- the KKT system of :9652-9664 with np.linalg.solve without guesses, the
min-norm correction of :9677 with np.linalg.pinv with them -- from a tau_full
and stacked body-frame Jacobians that do not come from the code under test.
None of it uses the closed form of the kernel.
"""
import numpy as np

import nimblephysics_amd as nimble

EPS = 0.01  # Skeleton.cpp:9643


def rig_world(fixed_first=False):
    """A free-root torso with two legs (revolute hip, revolute knee, a foot
    welded to the shin) and one arm on a UniversalJoint: 12 dofs, 8 bodies, 9
    device-model bodies (the arm's chain frame); the left knee has damping,
    stiffness and a rest position.  `fixed_first`: a fixed-base two-link
    pendulum skeleton is added before the rig, so the rig's root dofs start
    at 2."""
    from nimblephysics_amd import dynamics as D

    def tr(x, y, z):
        T = np.eye(4)
        T[:3, 3] = [x, y, z]
        return T

    def box(b, m, sx, sy, sz, com=(0.0, 0.0, 0.0)):
        b.setMass(m)
        b.setLocalCOM(com)
        b.setMomentOfInertia(m * (sy * sy + sz * sz) / 12, m * (sx * sx + sz * sz) / 12, m * (sx * sx + sy * sy) / 12)

    w = nimble.World()
    w.setGravity([0, -9.81, 0])
    if fixed_first:
        p = D.Skeleton("pendulum")
        j1, b1 = p.createRevoluteJointAndBodyNodePair(joint_name="p1", body_name="link1")
        j1.setAxis([0, 0, 1])
        j1.setTransformFromParentBodyNode(tr(2.0, 1.0, 0))
        j1.setTransformFromChildBodyNode(tr(0, 0.2, 0))
        box(b1, 0.7, 0.05, 0.4, 0.05)
        j2, b2 = p.createRevoluteJointAndBodyNodePair(b1, joint_name="p2", body_name="link2")
        j2.setAxis([1, 0, 0])
        j2.setTransformFromParentBodyNode(tr(0, -0.2, 0))
        j2.setTransformFromChildBodyNode(tr(0, 0.15, 0))
        j2.setDampingCoefficient(0, 0.2)
        box(b2, 0.4, 0.05, 0.3, 0.05)
        w.addSkeleton(p)
    rig = D.Skeleton("rig")
    _, torso = rig.createFreeJointAndBodyNodePair(body_name="torso")
    box(torso, 8.0, 0.3, 0.5, 0.2, com=(0.01, 0.05, -0.02))
    for side, x in (("l", 0.1), ("r", -0.1)):
        hip, thigh = rig.createRevoluteJointAndBodyNodePair(torso, joint_name=side + "_hip", body_name=side + "_thigh")
        hip.setAxis([1, 0, 0])
        hip.setTransformFromParentBodyNode(tr(x, -0.25, 0))
        hip.setTransformFromChildBodyNode(tr(0, 0.2, 0))
        box(thigh, 2.0, 0.1, 0.4, 0.1)
        knee, shin = rig.createRevoluteJointAndBodyNodePair(thigh, joint_name=side + "_knee", body_name=side + "_shin")
        knee.setAxis([1, 0, 0])
        knee.setTransformFromParentBodyNode(tr(0, -0.2, 0))
        knee.setTransformFromChildBodyNode(tr(0, 0.2, 0))
        box(shin, 1.5, 0.08, 0.4, 0.08)
        if side == "l":
            knee.setDampingCoefficient(0, 0.4)
            knee.setSpringStiffness(0, 3.0)
            knee.setRestPosition(0, -0.2)
        ankle, foot = rig.createWeldJointAndBodyNodePair(shin, joint_name=side + "_ankle", body_name=side + "_foot")
        ankle.setTransformFromParentBodyNode(tr(0, -0.2, 0))
        ankle.setTransformFromChildBodyNode(tr(0, 0.03, -0.05))
        box(foot, 0.5, 0.1, 0.06, 0.25)
    sh, arm = rig.createUniversalJointAndBodyNodePair(torso, joint_name="shoulder", body_name="arm")
    sh.setAxis1([0, 0, 1])
    sh.setAxis2([1, 0, 0])
    sh.setTransformFromParentBodyNode(tr(0.2, 0.2, 0))
    sh.setTransformFromChildBodyNode(tr(0, 0.25, 0))
    box(arm, 1.0, 0.06, 0.5, 0.06)
    w.addSkeleton(rig)
    return w


def rig_states(world, batch, seed=0):
    """Moderate random configurations and velocities (joint angles ~0.4 rad,
    the root within ~0.3 m of the origin), accelerations ~3 N(0, 1)."""
    rng = np.random.default_rng(seed)
    n = world.getNumDofs()
    q = 0.4 * rng.standard_normal((batch, n))
    v = 0.5 * rng.standard_normal((batch, n))
    a = 3.0 * rng.standard_normal((batch, n))
    return np.concatenate([q, v], axis=1), a


def reference(tau_full, J, r0, guesses=None):
    """(tau, F [k, 6], cond(N)) of one world from tau_full [n] and the stacked
    body-frame Jacobians J [6k, n] of the contact bodies, as the reference
    computes them; the six root dofs are r0 .. r0 + 5."""
    m6, n = J.shape
    jac_block = J[:, r0:r0 + 6].T  # [6, 6k]
    root = tau_full[r0:r0 + 6]
    w = np.ones(m6)
    if guesses is None:
        Bm = np.eye(m6)
        for i in range(m6 // 6):
            for c in (3, 4, 5):
                Bm[6 * i + c, 6 * i + c] = EPS
                w[6 * i + c] = 1.0 / EPS
        KKT = np.zeros((m6 + 6, m6 + 6))
        KKT[:m6, :m6] = Bm
        KKT[m6:, :m6] = jac_block
        KKT[:m6, m6:] = jac_block.T
        rhs = np.zeros(m6 + 6)
        rhs[m6:] = root
        F = np.linalg.solve(KKT, rhs)[:m6]
    else:
        f0 = np.asarray(guesses, dtype=np.float64).reshape(m6)
        F = np.linalg.pinv(jac_block) @ (root - jac_block @ f0) + f0
    tau = tau_full - J.T @ F
    tau[r0:r0 + 6] = 0.0
    N = jac_block @ np.diag(w) @ jac_block.T
    return tau, F.reshape(-1, 6), float(np.linalg.cond(N))
