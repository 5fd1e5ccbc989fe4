"""Batched differentiable inverse dynamics, mass matrix and bias forces.

``inverse_dynamics(world, state, ddq)`` answers "which joint forces produce
this motion?" for every world of a batch in one kernel launch:

    tau = ID(q, v, a) = M(q) a + C(q, v) - tau_ext(q) + D v + K (q - q0 + dt v)

-- the reference's Skeleton::getInverseDynamics (dart/dynamics/Skeleton.cpp:9433:
multiplyByImplicitMassMatrix :11124, getDampingForce :11355, getSpringForce
:11388, - getExternalForces()), taken over all of the world's dofs instead of
one skeleton's, in the conventions of ``timestep``: state = (q | v), for free
and ball joints v and a are the body-twist coordinates the step uses, C holds
gravity, tau_ext is the generalized force of ``body_wrench``.  tau is the
exact inverse of the contact-free step: ``timestep(world, state, tau)`` has
v' = v + dt a.  Contacts play no part -- a world with collision pairs gets
the answer it would get without them -- and tau is over all dofs, not the
action space.

state and ddq are float64 tensors, 1-D (one world) or 2-D [batch, ...]; CPU
tensors are staged to the current HIP device and the results come back on the
CPU, as in ``timestep``; there is no CPU compute path.  Nothing is stored in
the world and nothing of it is changed: no positions, velocities, control
forces, masses, stored wrenches or warm-start caches.

``mass`` as in ``timestep``: the world's getMassDims() tuned values, 1-D (one
vector for every world) or 2-D [B, getMassDims()] (one row per world), here
always expanded on the device to the kernels' per-world parameter array, so a
1-D mass does not go through World.setMasses either.  It is not
differentiable here: a ``mass`` that requires grad raises.  ``body_wrench``
and ``wrench_frame`` as in ``timestep``; the stored wrenches of the world's
bodies are not applied.

``body_inertia`` (instead of ``mass``): every body's ten inertial parameters
in INERTIA_FULL order (mass, local COM x y z, Ixx Iyy Izz Ixy Ixz Iyz), one
row per body in the world's body order (the order of ``body_wrench``):
[nBodies, 10], shared by the batch, or [B, nBodies, 10], one set per world.
It is differentiable; the gradient of a shared set is summed over the batch.
For a tuned mass vector: ``body_inertia=world.getBodyInertiaParameters(mass)``,
which autograd follows back to ``mass``.

Gradients (nimble_inverse_dynamics_backward), with g = dL/dtau:
    d/d ddq         M g
    d/d state       [(dID(q,v,a)/dq)^T g + K g,  (dC/dv)^T g + D g + dt K g]
    d/d body_wrench minus the world twist of body b under the rate vector g,
                    in the frame of the input
    d/d body_inertia (d tau / d theta)^T g
                    (nimble_invdyn_backward_inertia; the transposed
                    Skeleton::getJacobianOfID(ddq, wrt), Skeleton.cpp:1884, for
                    wrt = GROUP_MASSES, GROUP_COMS, GROUP_INERTIAS)

``inverse_dynamics_inertia_jacobian(world, state, ddq)`` is that matrix itself,
d tau / d theta [.., n, nBodies, 10] (getJacobianOfM + getJacobianOfC,
Skeleton.cpp:1832, :1779), for Gauss-Newton and least-squares fits of the
parameters; tau is affine in a body's mass and moments and quadratic in its
COM.  Not differentiable.

``mass_matrix(world, q)`` [.., n, n] and ``coriolis_and_gravity(world, state)``
[.., n] are World::getMassMatrix (dart/simulation/World.cpp:1974) and
World::getCoriolisAndGravityForces (World.cpp:1943) for a batch; both are
non-differentiable.
"""
from __future__ import annotations

from typing import Optional

import torch

from ._native import wrench_frame_flag
from .simulation import World
from .timestep import _compute_device


def _body_inertia(world: World, mass: Optional[torch.Tensor], B: int, cdev):
    """The kernels' per-world parameter array for `mass` (None: the model's
    own values, no array)."""
    if mass is None:
        return None
    D = world.getMassDims()
    if mass.dim() == 1:
        if mass.shape[0] != D:
            raise ValueError(f"mass must be a vector of the world's {D} tuned masses (World::tuneMass), got shape "
                             f"{tuple(mass.shape)}")
        mass = mass.reshape(1, D).expand(B, D)
    elif mass.dim() != 2 or tuple(mass.shape) != (B, D):
        raise ValueError(f"per-world mass must be [{B}, {D}] (batch, the world's tuned mass dims), got "
                         f"{tuple(mass.shape)}")
    return world._batched_inertia(mass.detach().to(cdev, torch.float64).contiguous())


def _body_inertia_shared(world: World, body_inertia: torch.Tensor, state: torch.Tensor) -> bool:
    """Checks the shape of `body_inertia` for this state (before anything
    touches a device); True when it is one set [nBodies, 10] for the batch."""
    nbw = world.getNumBodyNodes()
    shape = tuple(body_inertia.shape)
    shared = body_inertia.dim() == 2
    if shape[-2:] != (nbw, 10) or body_inertia.dim() not in (2, 3) or (state.dim() == 1 and not shared):
        want = f"[{nbw}, 10]" if state.dim() == 1 else f"[{nbw}, 10] or [{state.shape[0]}, {nbw}, 10]"
        raise ValueError(f"body_inertia must be {want} for this state (INERTIA_FULL order per body of the world), "
                         f"got {shape}")
    if not shared and shape[0] != state.shape[0]:
        raise ValueError(f"per-world body_inertia must be [{state.shape[0]}, {nbw}, 10] for this state, got {shape}")
    return shared


def _stage_body_inertia(world: World, body_inertia: torch.Tensor, shared: bool, B: int, cdev):
    """The kernels' per-world parameter array [B, num_bodies, 10] for
    `body_inertia` in the world's body order."""
    p = body_inertia.detach().to(cdev, torch.float64)
    if shared:
        p = p.unsqueeze(0).expand(B, *p.shape)
    return world._scatter_inertia(p).contiguous()


def _stage(world: World, state: torch.Tensor, ddq: Optional[torch.Tensor], cdev):
    """2-D contiguous float64 device copies of state (and ddq)."""
    n = world.getNumDofs()
    squeeze = state.dim() == 1
    st = state.detach().to(cdev, torch.float64)
    st = (st.reshape(1, -1) if squeeze else st).contiguous()
    if st.dim() != 2 or st.shape[1] != 2 * n:
        raise ValueError(f"state has {st.shape[-1]} columns, world expects {2 * n}")
    if ddq is None:
        return squeeze, st, None
    if ddq.dim() != state.dim():
        raise ValueError("state and ddq must both be 1-D or both 2-D")
    a = ddq.detach().to(cdev, torch.float64)
    a = (a.reshape(1, -1) if squeeze else a).contiguous()
    if tuple(a.shape) != (st.shape[0], n):
        raise ValueError(f"ddq must be {[st.shape[0], n]} for this state, got {list(a.shape)}")
    return squeeze, st, a


class InverseDynamicsLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, world: World, state: torch.Tensor, ddq: torch.Tensor, mass: Optional[torch.Tensor],
                body_wrench: Optional[torch.Tensor] = None, wrench_frame="world",
                body_inertia: Optional[torch.Tensor] = None):
        if mass is not None and body_inertia is not None:
            raise ValueError("inverse_dynamics: give mass or body_inertia, not both")
        if mass is not None and mass.requires_grad:
            raise ValueError("inverse_dynamics: mass is not differentiable here (detach it, pass "
                             "body_inertia=world.getBodyInertiaParameters(mass), or differentiate through timestep)")
        frame = wrench_frame_flag(wrench_frame)
        if body_wrench is not None:
            want = (world.getNumBodyNodes(), 6) if state.dim() == 1 else (state.shape[0], world.getNumBodyNodes(), 6)
            if tuple(body_wrench.shape) != want:
                raise ValueError(f"body_wrench must be {list(want)} for this state ([torque xyz, force xyz] per body "
                                 f"of the world), got {tuple(body_wrench.shape)}")
            ctx.wrench_device = body_wrench.device
        ctx.inertia_shared = False
        if body_inertia is not None:
            ctx.inertia_shared = _body_inertia_shared(world, body_inertia, state)
            ctx.inertia_device = body_inertia.device
        ctx.out_device = state.device
        cdev = _compute_device(state)
        with torch.cuda.device(cdev):
            squeeze, st, a = _stage(world, state, ddq, cdev)
            B = st.shape[0]
            bi = _body_inertia(world, mass, B, cdev)
            if body_inertia is not None:
                bi = _stage_body_inertia(world, body_inertia, ctx.inertia_shared, B, cdev)
            bw = None
            if body_wrench is not None:
                w3 = body_wrench.detach().to(cdev, torch.float64)
                bw = world._scatter_wrench(w3.unsqueeze(0) if squeeze else w3)
            dev = world.native(cdev)
            tau = torch.empty_like(a)
            stream = torch.cuda.current_stream(cdev).cuda_stream
            dev.inverse_dynamics(st, a, tau, stream, body_inertia=bi, body_wrench=bw, wrench_frame=frame)
        ctx.world = world
        ctx.dev = dev  # the backward runs on the model of the forward
        ctx.squeeze = squeeze
        ctx.body_inertia = bi
        ctx.body_wrench = bw
        ctx.wrench_frame = frame
        ctx.save_for_backward(st, a)
        return (tau[0] if squeeze else tau).to(ctx.out_device)

    @staticmethod
    def backward(ctx, grad_tau):
        st, a = ctx.saved_tensors
        dev = ctx.dev
        if dev.h is None:
            raise RuntimeError("the world model that produced this result was released before backward")
        with torch.cuda.device(st.device):
            g = grad_tau.detach().reshape(a.shape).to(st.device, torch.float64).contiguous()
            gs = torch.empty_like(st)
            ga = torch.empty_like(a)
            bw = ctx.body_wrench
            gw = torch.empty_like(bw) if bw is not None and ctx.needs_input_grad[4] else None
            # (a body_inertia that does not require grad: the entry point without grad_inertia)
            gi = torch.empty_like(ctx.body_inertia) if ctx.needs_input_grad[6] else None
            stream = torch.cuda.current_stream(st.device).cuda_stream
            dev.inverse_dynamics_backward(st, a, g, gs, ga, stream, body_inertia=ctx.body_inertia, body_wrench=bw,
                                          wrench_frame=ctx.wrench_frame, grad_wrench=gw, grad_inertia=gi)
        od = ctx.out_device
        if gw is not None:
            gw = ctx.world._gather_wrench(gw)
            gw = (gw[0] if ctx.squeeze else gw).to(ctx.wrench_device)
        if gi is not None:
            gi = ctx.world._gather_inertia(gi)
            gi = (gi.sum(0) if ctx.inertia_shared else gi).to(ctx.inertia_device)
        if ctx.squeeze:
            return None, gs[0].to(od), ga[0].to(od), None, gw, None, gi
        return None, gs.to(od), ga.to(od), None, gw, None, gi


def inverse_dynamics(world: World, state: torch.Tensor, ddq: torch.Tensor, mass: Optional[torch.Tensor] = None,
                     body_wrench: Optional[torch.Tensor] = None, wrench_frame="world",
                     body_inertia: Optional[torch.Tensor] = None) -> torch.Tensor:
    """tau = ID(q, v, a), differentiable in state, ddq, body_wrench and
    body_inertia; see the module docstring."""
    return InverseDynamicsLayer.apply(world, state, ddq, mass, body_wrench, wrench_frame, body_inertia)


def inverse_dynamics_inertia_jacobian(world: World, state: torch.Tensor, ddq: torch.Tensor,
                                      body_inertia: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d tau / d theta: [n, nBodies, 10] for a 1-D state, [B, n, nBodies, 10]
    for [B, 2n]; bodies in the world's body order, parameters in INERTIA_FULL
    order (Skeleton::getJacobianOfID(ddq, wrt), Skeleton.cpp:1884, for wrt =
    GROUP_MASSES, GROUP_COMS and GROUP_INERTIAS, for a batch).  body_inertia
    as in inverse_dynamics.  Exactly 0 where the dof is neither the body's nor
    one of its ancestors'.  Not differentiable."""
    n = world.getNumDofs()
    if state.dim() not in (1, 2) or state.shape[-1] != 2 * n:
        raise ValueError(f"state has {state.shape[-1]} columns, world expects {2 * n}")
    if ddq.dim() != state.dim() or tuple(ddq.shape) != tuple(state.shape[:-1]) + (n,):
        raise ValueError(f"ddq must be {list(state.shape[:-1]) + [n]} for this state, got {list(ddq.shape)}")
    shared = body_inertia is not None and _body_inertia_shared(world, body_inertia, state)
    out_device = state.device
    cdev = _compute_device(state)
    with torch.cuda.device(cdev):
        squeeze, st, a = _stage(world, state, ddq, cdev)
        B = st.shape[0]
        bi = None
        if body_inertia is not None:
            bi = _stage_body_inertia(world, body_inertia, shared, B, cdev)
        dev = world.native(cdev)
        J = torch.empty((B, n, dev.nb, 10), dtype=torch.float64, device=cdev)
        dev.inverse_dynamics_inertia_jacobian(st, a, J, torch.cuda.current_stream(cdev).cuda_stream, body_inertia=bi)
        J = world._gather_inertia(J)
    return (J[0] if squeeze else J).to(out_device)


def _queries(world: World, state: torch.Tensor, want_mass: bool, want_bias: bool):
    """One forward launch at ddq = 0 for the two batched getters."""
    out_device = state.device
    cdev = _compute_device(state)
    with torch.cuda.device(cdev):
        squeeze, st, _ = _stage(world, state, None, cdev)
        B, n = st.shape[0], world.getNumDofs()
        a = torch.zeros((B, n), dtype=torch.float64, device=cdev)
        tau = torch.empty_like(a)
        M = torch.empty((B, n, n), dtype=torch.float64, device=cdev) if want_mass else None
        C = torch.empty((B, n), dtype=torch.float64, device=cdev) if want_bias else None
        dev = world.native(cdev)
        dev.inverse_dynamics(st, a, tau, torch.cuda.current_stream(cdev).cuda_stream, mass_matrix=M, bias=C)
    out = M if want_mass else C
    return (out[0] if squeeze else out).to(out_device)


def mass_matrix(world: World, q: torch.Tensor) -> torch.Tensor:
    """M(q), full symmetric: [n, n] for a 1-D q [n], [B, n, n] for [B, n]
    (World::getMassMatrix, World.cpp:1974, for a batch).  Not differentiable."""
    n = world.getNumDofs()
    if q.shape[-1] != n:
        raise ValueError(f"q has {q.shape[-1]} columns, world has {n} dofs")
    state = torch.cat([q.detach(), torch.zeros_like(q.detach())], dim=-1)
    return _queries(world, state, True, False)


def coriolis_and_gravity(world: World, state: torch.Tensor) -> torch.Tensor:
    """C(q, v) with gravity, without damping, spring or external forces: [n]
    for a 1-D state [2n], [B, n] for [B, 2n]
    (World::getCoriolisAndGravityForces, World.cpp:1943, for a batch).  Not
    differentiable."""
    return _queries(world, state, False, True)
