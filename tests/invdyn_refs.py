"""CPU references for the inverse-dynamics tests (test infrastructure), all
from the existing oracle (oracle.OracleWorld), none from the code under test:

* values: tau_ref = M(q) a + C(q, v) + D v + K (q - q0 + dt v) from
  oracle_mass_matrix / oracle_coriolis_gravity (pinned to closed forms in
  tests/test_dynamics_closed_form.py) and the description's damping, spring
  and rest positions;
* analytic Jacobian: the oracle stepped contact-free from (q, v) with forces
  tau_ref has a* = a, and its analytic step Jacobian J (getStateJacobian)
  gives, with Jv = J[n:, :],
      dID/dq = -M Jv[:, :n] / dt,  dID/dv = M (I - Jv[:, n:]) / dt,  dID/da = M;
* second reference: Richardson-extrapolated central differences of tau_ref,
  (4 J(h/2) - J(h)) / 3 with h = 2e-3 (plain central differences at
  h <= 1e-5 carry 2e-7 .. 4e-5 of rounding error on the Atlas and cannot
  certify 1e-6).
"""
import numpy as np

from oracle import oracle as O

H = 2e-3


class Ref:
    def __init__(self, world):
        d = world.desc_arrays()
        self.o = O.OracleWorld(world)
        self.n = world.getNumDofs()
        self.dt = float(d["dt"])
        self.D = np.asarray(d["damping"], dtype=np.float64)
        self.K = np.asarray(d["spring"], dtype=np.float64)
        self.q0 = np.asarray(d["rest_position"], dtype=np.float64)

    def passive(self, q, v):
        return self.D * v + self.K * (q - self.q0 + self.dt * v)

    def tau(self, q, v, a):
        return self.o.mass_matrix(q) @ a + self.o.coriolis_gravity(q, v) + self.passive(q, v)

    def tau_batch(self, st, a):
        n = self.n
        return np.stack([self.tau(s[:n], s[n:], x) for s, x in zip(st, a)])

    def analytic(self, q, v, a):
        """(dID/dq, dID/dv, dID/da) [n, n] each, from the oracle's analytic
        step Jacobian; the world must be contact-free at (q, v)."""
        n, dt = self.n, self.dt
        tau = self.tau(q, v, a)
        nxt = self.o.forward(np.concatenate([q, v])[None], tau[None])
        assert self.o.num_contacts(0) == 0
        # the round trip the construction rests on: a* = a
        assert np.abs(nxt[0, n:] - (v + dt * a)).max() <= 1e-9 * max(1.0, np.abs(v + dt * a).max())
        J, _ = self.o.jacobians()
        Jv = J[0, n:, :]
        M = self.o.mass_matrix(q)
        return -M @ Jv[:, :n] / dt, M @ (np.eye(n) - Jv[:, n:]) / dt, M

    def richardson(self, q, v, a, fn=None):
        """(dID/dq, dID/dv, dID/da) by Richardson-extrapolated central
        differences of `fn` (default: tau_ref)."""
        fn = fn or self.tau
        n = self.n
        x0 = np.concatenate([q, v, a])

        def central(h):
            J = np.zeros((n, 3 * n))
            for k in range(3 * n):
                xp, xm = x0.copy(), x0.copy()
                xp[k] += h
                xm[k] -= h
                J[:, k] = (fn(xp[:n], xp[n:2 * n], xp[2 * n:]) - fn(xm[:n], xm[n:2 * n], xm[2 * n:])) / (2 * h)
            return J

        J = (4.0 * central(H / 2) - central(H)) / 3.0
        return J[:, :n], J[:, n:2 * n], J[:, 2 * n:]


def damped_cartpole():
    """The cartpole with non-zero damping, stiffness and rest position on
    every dof, set through the Joint setters."""
    import models
    w = models.cartpole_world()
    k = 0
    for s in w.skeletons:
        for b in s.bodies:
            j = b.joint
            for i in range(j.getNumDofs()):
                j.setDampingCoefficient(i, 0.3 + 0.2 * k)
                j.setSpringStiffness(i, 2.0 + k)
                j.setRestPosition(i, 0.1 - 0.25 * k)
                k += 1
    d = w.desc_arrays()
    assert k == w.getNumDofs()
    assert np.all(d["damping"] != 0) and np.all(d["spring"] != 0) and np.all(d["rest_position"] != 0)
    return w


def accelerations(shape, seed):
    """a ~ 3 N(0, 1)"""
    return 3.0 * np.random.default_rng(seed).standard_normal(shape)


def desc_lines(world):
    """The world description in the text format of tests/cpp/wave_emu's
    drivers (see step_emu.cpp)."""
    import wave_emu
    f = wave_emu._fmt
    d = world.desc_arrays()
    cand = np.asarray(d.get("mesh_vertex_candidate", []))
    nmv = len(np.asarray(d["mesh_vertices"])) // 3
    lines = [f([d["num_bodies"], d["num_dofs"], d["num_shapes"], nmv, d["penetration_correction"],
                d["parallel_pos_vel"], 1 if len(cand) else 0], True),
             f([d["dt"], *d["gravity"], d["contact_clipping_depth"], d["fallback_cfm"]])]
    for k in ("parent", "skeleton", "joint_type", "dof_offset", "skeleton_mobile"):
        lines.append(f(d[k], True))
    for k in ("T_parent_joint", "T_child_joint", "axis", "mass", "com", "moment", "friction", "restitution",
              "damping", "spring", "rest_position", "pos_lower", "pos_upper", "vel_lower", "vel_upper",
              "force_lower", "force_upper"):
        lines.append(f(d[k]))
    lines += [f(d["shape_body"], True), f(d["shape_type"], True), f(d["shape_size"]), f(d["shape_T"]),
              f(d["shape_mesh_first"], True), f(d["shape_mesh_count"], True), f(d["mesh_vertices"])]
    if len(cand):
        lines.append(f(cand, True))
    return lines
