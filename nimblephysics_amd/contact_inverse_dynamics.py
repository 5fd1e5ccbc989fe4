"""Batched contact inverse dynamics: joint torques and contact wrenches.

``contact_inverse_dynamics(world, state, ddq, contact_bodies)`` answers, for
every world of a batch in one kernel launch, "which joint torques, and which
wrenches on these bodies, produce this motion?" for a floating-base skeleton
whose six root dofs are not actuated -- the reference's
Skeleton::getContactInverseDynamics (dart/dynamics/Skeleton.cpp:9449, one
body) and Skeleton::getMultipleContactInverseDynamics (:9578).

With tau_full = ``inverse_dynamics(world, state, ddq, ...)``, r its rows at the
skeleton's six root dofs and J_i the body-frame Jacobian of contact body i,
the wrenches F_i ([torque xyz, force xyz] in body i's own frame) satisfy
sum_i J_i^T F_i = r in the root rows, and

    tau = tau_full - sum_i J_i^T F_i,   exactly 0.0 in the six root rows.

The dofs of other skeletons keep tau_full.  One body determines its wrench.
With several, ``wrench_guesses`` [.., k, 6] selects the solution nearest the
guesses; without them the solution with the smallest moments is taken (the
reference's weighting: 1 on torque, 0.01 on force components).

``contact_bodies`` is a list of 1 .. 8 distinct BodyNodes of one skeleton of
the world whose root joint is a FreeJoint.  state, ddq, ``mass``,
``body_wrench`` (known further wrenches) and ``wrench_frame`` as in
``inverse_dynamics``: 1-D (one world) or 2-D [batch, ...] float64 tensors, CPU
tensors are staged to the device and the results come back on the CPU, the
stored wrenches of the world's bodies are not applied.  Contacts of the
collision detector play no part.

The outputs are not differentiable (as in the reference, and as
``mass_matrix``): inputs that require grad are accepted and the outputs come
back detached.  For gradients pass the wrenches on to the differentiable call,
``inverse_dynamics(world, state, ddq, body_wrench=W, wrench_frame="body")``
with W zero but for the rows of the contact bodies, which returns the same tau
outside the root rows.

dynamics.Skeleton.getContactInverseDynamics / getMultipleContactInverseDynamics
are the reference's surface on top of this, at the world's current state.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import dynamics as dyn
from ._native import MAX_CONTACT_BODIES, wrench_frame_flag
from .inverse_dynamics import _body_inertia, _stage
from .simulation import World
from .timestep import _compute_device


def contact_body_indices(world: World, contact_bodies: Sequence["dyn.BodyNode"]):
    """Device-model index of each contact body (World._model_bodies: the
    massless frames of compound-joint chains shift the indices), after the
    checks that need no device."""
    bodies = list(contact_bodies)
    if len(bodies) == 0:
        raise ValueError("contact_inverse_dynamics needs at least one contact body")
    if len(bodies) > MAX_CONTACT_BODIES:
        raise ValueError(f"{len(bodies)} contact bodies: at most {MAX_CONTACT_BODIES} are supported")
    index = {id(e[2]): i for i, e in enumerate(world._model_bodies()) if e[2] is not None}
    out = []
    for b in bodies:
        if id(b) not in index:
            raise ValueError(f"contact body {getattr(b, 'name', b)!r} is not a BodyNode of this world")
        if index[id(b)] in out:
            raise ValueError(f"duplicate contact body {b.name!r}")
        out.append(index[id(b)])
    skel = bodies[0].skel
    if any(b.skel is not skel for b in bodies):
        raise ValueError("the contact bodies belong to different skeletons")
    if skel.bodies[0].joint.kind != dyn.JOINT_FREE:
        raise ValueError(f"skeleton {skel.name!r} has no FreeJoint at its root: its root dofs cannot be left "
                         "unactuated")
    return out


def contact_inverse_dynamics(world: World, state: torch.Tensor, ddq: torch.Tensor, contact_bodies,
                             wrench_guesses: Optional[torch.Tensor] = None, mass: Optional[torch.Tensor] = None,
                             body_wrench: Optional[torch.Tensor] = None, wrench_frame="world"):
    """(tau, contact_wrenches): tau [.., n] with the root's six rows 0.0 and
    contact_wrenches [.., k, 6] in each body's own frame; see the module
    docstring."""
    idx = contact_body_indices(world, contact_bodies)
    k = len(idx)
    frame = wrench_frame_flag(wrench_frame)
    if state.dim() not in (1, 2) or ddq.dim() != state.dim():
        raise ValueError("state and ddq must both be 1-D or both 2-D")
    lead = () if state.dim() == 1 else (state.shape[0],)
    if wrench_guesses is not None and tuple(wrench_guesses.shape) != lead + (k, 6):
        raise ValueError(f"wrench_guesses must be {list(lead + (k, 6))} (one body-frame [torque xyz, force xyz] per "
                         f"contact body), got {tuple(wrench_guesses.shape)}")
    if body_wrench is not None and tuple(body_wrench.shape) != lead + (world.getNumBodyNodes(), 6):
        raise ValueError(f"body_wrench must be {list(lead + (world.getNumBodyNodes(), 6))} for this state ([torque "
                         f"xyz, force xyz] per body of the world), got {tuple(body_wrench.shape)}")
    out_device = state.device
    cdev = _compute_device(state)
    with torch.cuda.device(cdev):
        squeeze, st, a = _stage(world, state, ddq, cdev)
        B = st.shape[0]
        bi = _body_inertia(world, mass, B, cdev)
        bw = None
        if body_wrench is not None:
            w3 = body_wrench.detach().to(cdev, torch.float64)
            bw = world._scatter_wrench(w3.unsqueeze(0) if squeeze else w3)
        F0 = None
        if wrench_guesses is not None:
            F0 = wrench_guesses.detach().to(cdev, torch.float64).reshape(B, k, 6).contiguous()
        dev = world.native(cdev)
        tau = torch.empty_like(a)
        F = torch.empty((B, k, 6), dtype=torch.float64, device=cdev)
        dev.contact_inverse_dynamics(st, a, idx, tau, F, torch.cuda.current_stream(cdev).cuda_stream,
                                     wrench_guesses=F0, body_inertia=bi, body_wrench=bw, wrench_frame=frame)
    if squeeze:
        tau, F = tau[0], F[0]
    return tau.to(out_device), F.to(out_device)


class _ContactInverseDynamicsResultBase:
    """What the two results share: the motion, the joint torques and the
    check of the reference's sumError()."""

    def _sum_error(self, wrenches) -> float:
        """|| M^-1 (ID(acc; contact wrenches) - jointTorques) || over the
        skeleton's dofs: the dynamics are linear in the accelerations, so this
        is the reference's || realAcc - acc || (forward dynamics of
        jointTorques under the contact wrenches against acc)."""
        from .inverse_dynamics import inverse_dynamics, mass_matrix
        skel, world = self.skel, self.skel.world
        lo, hi = _skeleton_dofs(world, skel)
        q, v, a = _world_vectors(world, skel, self.pos, self.vel, self.acc)
        W = np.zeros((world.getNumBodyNodes(), 6)) if self._ext is None else self._ext.copy()
        order = {id(b): i for i, b in enumerate(world._world_bodies())}
        for b, f in wrenches:
            W[order[id(b)]] += f
        t = torch.as_tensor
        full = inverse_dynamics(world, t(np.concatenate([q, v])), t(a), body_wrench=t(W), wrench_frame="body").numpy()
        M = mass_matrix(world, t(q)).numpy()[lo:hi, lo:hi]
        return float(np.linalg.norm(np.linalg.solve(M, full[lo:hi] - self.jointTorques)))


class ContactInverseDynamicsResult(_ContactInverseDynamicsResultBase):
    """Skeleton::ContactInverseDynamicsResult (dart/dynamics/Skeleton.hpp)."""

    def __init__(self, skel, contactBody, pos, vel, acc, contactWrench, jointTorques, ext=None):
        self._ext = ext  # the bodies' stored wrenches the result was computed under
        self.skel, self.contactBody = skel, contactBody
        self.pos, self.vel, self.acc = pos, vel, acc
        self.contactWrench, self.jointTorques = contactWrench, jointTorques

    def sumError(self) -> float:
        return self._sum_error([(self.contactBody, self.contactWrench)])


class MultipleContactInverseDynamicsResult(_ContactInverseDynamicsResultBase):
    """Skeleton::MultipleContactInverseDynamicsResult (Skeleton.hpp)."""

    def __init__(self, skel, contactBodies, pos, vel, acc, contactWrenches, contactWrenchGuesses, jointTorques,
                 ext=None):
        self._ext = ext
        self.skel, self.contactBodies = skel, contactBodies
        self.pos, self.vel, self.acc = pos, vel, acc
        self.contactWrenches, self.contactWrenchGuesses = contactWrenches, contactWrenchGuesses
        self.jointTorques = jointTorques

    def sumError(self) -> float:
        return self._sum_error(list(zip(self.contactBodies, self.contactWrenches)))


def _skeleton_dofs(world: World, skel):
    if world is None or not any(s is skel for s in world.skeletons):
        raise ValueError(f"skeleton {skel.name!r} is in no world: the device model is the world's")
    lo = 0
    for s in world.skeletons:
        if s is skel:
            break
        lo += s.getNumDofs()
    return lo, lo + skel.getNumDofs()


def _world_vectors(world: World, skel, pos, vel, acc):
    """World-sized q, v, a with the skeleton's own values in its rows; the
    other skeletons at the world's state with ddq = 0."""
    lo, hi = _skeleton_dofs(world, skel)
    q, v, a = world.getPositions(), world.getVelocities(), np.zeros(world.getNumDofs())
    q[lo:hi], v[lo:hi], a[lo:hi] = pos, vel, acc
    return q, v, a


def skeleton_contact_inverse_dynamics(skel, accelerations, bodies, guesses):
    """The work of the two Skeleton methods: the functional call at the
    world's current positions and velocities with the bodies' stored wrenches
    applied (the reference's `- getExternalForces()`), accelerations and
    torques over the skeleton's own dofs.  Returns (pos, vel, acc, tau,
    wrenches [k, 6], the stored wrenches or None)."""
    world = skel.world
    lo, hi = _skeleton_dofs(world, skel)
    acc = np.asarray(accelerations, dtype=np.float64).reshape(-1)
    if acc.shape[0] != hi - lo:
        raise ValueError(f"accelerations must have the skeleton's {hi - lo} dofs, got {acc.shape[0]}")
    bodies = list(bodies)
    if any(getattr(b, "skel", None) is not skel for b in bodies):
        raise ValueError(f"a contact body does not belong to skeleton {skel.name!r}")
    pos, vel = skel.getPositions(), skel.getVelocities()
    q, v, a = _world_vectors(world, skel, pos, vel, acc)
    t = torch.as_tensor
    F0 = None
    if len(guesses) > 0:
        F0 = t(np.asarray(guesses, dtype=np.float64).reshape(-1, 6))
    stored = world._stored_wrench()
    tau, F = contact_inverse_dynamics(world, t(np.concatenate([q, v])), t(a), bodies, wrench_guesses=F0,
                                      body_wrench=None if stored is None else t(stored), wrench_frame="body")
    return pos, vel, acc, tau.numpy()[lo:hi].copy(), F.numpy().copy(), stored
