"""CPU references for the inertial-parameter derivatives of the inverse
dynamics (test infrastructure), all from the existing oracle, none from the
code under test.

tau_ref(theta) = invdyn_refs.Ref(world).tau on a world whose bodies were set
to the parameter rows theta with per_world_params.set_world_params.  tau is a
polynomial in theta -- affine in a body's mass and moments, quadratic in its
COM, cubic jointly -- so

* a column d tau / d theta_{b,p} by central differences is exact up to
  rounding for ANY step; the steps are large (0.25 x the body's mass, 0.05 m
  per COM component, 0.25 x the body's smallest diagonal moment per moment
  entry, but see MOMENT_STEP_FLOOR), which keeps the rounding error of the
  difference small;
* along a direction that moves all parameters at once,
  (4 c(h/2) - c(h)) / 3 with h = 1 is exact as well (c = central difference).

case() also returns the guard of the bar: the columns at the steps above
against the columns at half of them (`half`), and the Richardson directional
difference against J d (`rich`), under _rel; the device tests assert both at
1e-7 before they compare the device against J.
"""
import functools

import numpy as np

import invdyn_refs
import models
import per_world_params

B = 3

# The smallest step of a moment entry, kg m^2.  A column's rounding error is
# that of tau over the step, about 2^-52 |tau| / h.  The Atlas' own values
# (parameter set 0) hold bodies with moments of 1e-5 kg m^2: 0.25 x that is a
# step of 2.5e-6, and with |tau| up to 490 the columns at h and h / 2 then
# differ by 5.7e-9, 1.2e-6 under _rel (floor 1e-5 x 490) -- twelve times the
# 1e-7 the reference has to hold before anything is compared against it.
# 1e-7 x 4.9e-3 needs h >= 2e-4; 1e-3 leaves a factor of five (measured:
# 1.7e-8).  Below the floor a step takes such a body's moment out of the
# positive definite cone; the oracle's tau = M a + C is the same polynomial
# there (no factorisation is involved), and the two guards -- h against h / 2,
# Richardson against J d -- are what certify the columns.
MOMENT_STEP_FLOOR = 1e-3


def steps(P):
    """[nb, 10]: the difference step of every parameter of the rows P; zero
    rows (the massless frames of compound-joint chains) get zero steps."""
    h = np.zeros_like(P)
    h[:, 0] = 0.25 * P[:, 0]
    h[:, 1:4] = 0.05
    h[:, 4:10] = np.maximum(0.25 * P[:, 4:7].min(axis=1)[:, None], MOMENT_STEP_FLOOR)
    h[P[:, 0] == 0] = 0.0
    return h


def massive(world):
    """Device-model indices of the bodies that are BodyNodes of the world."""
    return [i for i, e in enumerate(world._model_bodies()) if e[2] is not None]


class TauOfTheta:
    """tau_ref as a function of the [nb, 10] parameter rows at fixed (q, v, a);
    restore() puts the world's own values back."""

    def __init__(self, world, q, v, a):
        self.world, self.q, self.v, self.a = world, q, v, a
        self.base = per_world_params.base_params(world)
        self.evals = 0

    def __call__(self, P):
        per_world_params.set_world_params(self.world, P)
        self.evals += 1
        return invdyn_refs.Ref(self.world).tau(self.q, self.v, self.a)

    def restore(self):
        per_world_params.set_world_params(self.world, self.base)


def columns(f, P, bodies, scale=1.0):
    """J [n, nb, 10]: central differences of f at P with steps `scale` x
    steps(P), for the listed bodies (zero elsewhere)."""
    h = steps(P) * scale
    J = None
    for b in bodies:
        for p in range(10):
            Pp, Pm = P.copy(), P.copy()
            Pp[b, p] += h[b, p]
            Pm[b, p] -= h[b, p]
            col = (f(Pp) - f(Pm)) / (2 * h[b, p])
            if J is None:
                J = np.zeros((col.shape[0], P.shape[0], 10))
            J[:, b, p] = col
    return J


def richardson_direction(f, P, d):
    """(4 c(1/2) - c(1)) / 3 of f along d [nb, 10]: exact for a cubic."""
    c = lambda h: (f(P + h * d) - f(P - h * d)) / (2 * h)  # noqa: E731
    return (4.0 * c(0.5) - c(1.0)) / 3.0


def _world(name):
    if name == "cartpole":
        w = invdyn_refs.damped_cartpole()
        st, _ = models.random_states(w, B, seed=3, q_scale=0.5, v_scale=1.0)
    elif name == "ball":
        w = models.ball_world(ground=False)
        st, _ = models.ball_states(B, seed=21, contact=False)
    elif name == "compound":
        w = models.compound_world(ground=False)
        st, _ = models.compound_states(B, seed=21, contact=False)
    elif name == "atlas":
        w = models.atlas_world(False)
        st, _ = models.random_states(w, B, seed=3, q_scale=0.2, v_scale=0.3)
    else:
        raise KeyError(name)
    return w, st


def case_bodies(name, world, b):
    """The bodies whose columns are compared on world b: all of them, but on
    the Atlas' second and third world the first two, the middle and the last."""
    m = massive(world)
    if name == "atlas" and b > 0:
        return [m[0], m[1], m[len(m) // 2], m[-1]]
    return m


@functools.lru_cache(maxsize=None)
def case(name, worlds=B):
    """One model's inputs and references, computed once and shared (treat as
    read-only): a dict with world (fresh, its own values), st [B, 2n],
    a [B, n], P [B, nb, 10] (world b on parameter set b % 3), bodies[b], J[b]
    [n, nb, 10] (oracle columns of the listed bodies), and the guard figures
    half (columns at the steps vs half steps) and rich (Richardson directional
    difference vs J d), maxima under _rel over the worlds."""
    from test_gpu_contact_parity import _rel
    w, st = _world(name)
    st = st[:worlds]
    n = w.getNumDofs()
    a = invdyn_refs.accelerations((worlds, n), seed=5)
    P = per_world_params.batch_params(w, worlds)
    ow, _ = _world(name)  # the oracle's world: its bodies are rewritten
    out = {"world": w, "st": st, "a": a, "P": P, "bodies": [], "J": [], "half": 0.0, "rich": 0.0}
    for b in range(worlds):
        f = TauOfTheta(ow, st[b, :n], st[b, n:], a[b])
        bodies = case_bodies(name, ow, b)
        J = columns(f, P[b], bodies)
        Jh = columns(f, P[b], bodies, 0.5)
        d = np.zeros_like(P[b])
        d[bodies] = steps(P[b])[bodies]
        r = richardson_direction(f, P[b], d)
        f.restore()
        out["half"] = max(out["half"], _rel(Jh, J))
        out["rich"] = max(out["rich"], _rel(np.einsum("jbp,bp->j", J, d), r))
        out["bodies"].append(bodies)
        out["J"].append(J)
    return out
