"""The fixed per-world body parameter sets of the per-world inertia tests.

`param_sets(world)` gives K = 3 arrays [nb, 10] (device-model bodies, ten
values each in INERTIA_FULL order: mass, local COM x y z, Ixx Iyy Izz Ixy Ixz
Iyz) built from the model's own values:

    set 0   the model's values, unchanged
    set 1   mass x 0.8, COM + (2, -1, 0.5) cm, diagonal moments x 1.2,
            Ixy = +5 % of the smallest (scaled) diagonal, Ixz = Iyz = 0
    set 2   mass x 1.3, COM + (-1.5, 2, -2) cm, diagonal moments x 0.7,
            Ixz = -5 %, Iyz = +5 % of the smallest diagonal, Ixy = 0

Every set keeps every massive body's moment positive definite: the
off-diagonal entries of a row sum to at most 10 % of the smallest diagonal
entry, so the matrix is strictly diagonally dominant with a positive
diagonal.  The massless frames of compound-joint chains stay all zero.
World b of a batch gets set b % 3.
"""
import numpy as np

K = 3
_MASS = (1.0, 0.8, 1.3)
_COM = ((0.0, 0.0, 0.0), (0.02, -0.01, 0.005), (-0.015, 0.02, -0.02))
_DIAG = (1.0, 1.2, 0.7)
_OFF = (None, (0.05, 0.0, 0.0), (0.0, -0.05, 0.05))


def base_params(world):
    """[nb, 10]: the model's own values per device body."""
    return world._body_inertia_base()


def param_sets(world):
    base = base_params(world)
    out = []
    for k in range(K):
        P = base.copy()
        massive = base[:, 0] > 0
        P[:, 0] = base[:, 0] * _MASS[k]
        P[massive, 1:4] = base[massive, 1:4] + np.array(_COM[k])
        P[:, 4:7] = base[:, 4:7] * _DIAG[k]
        if _OFF[k] is not None:
            P[:, 7:10] = P[:, 4:7].min(axis=1)[:, None] * np.array(_OFF[k])
        out.append(P)
    return out


def positive_definite(P):
    """Every massive body of the [nb, 10] array has a positive mass and a
    positive definite moment."""
    for row in P:
        if row[0] == 0 and not row[4:].any():
            continue
        Ixx, Iyy, Izz, Ixy, Ixz, Iyz = row[4:]
        I = np.array([[Ixx, Ixy, Ixz], [Ixy, Iyy, Iyz], [Ixz, Iyz, Izz]])
        if row[0] <= 0 or np.linalg.eigvalsh(I).min() <= 0:
            return False
    return True


def batch_params(world, B):
    """[B, nb, 10]: world b gets set b % 3."""
    sets = param_sets(world)
    return np.stack([sets[b % K] for b in range(B)])


def set_world_params(world, P):
    """Write the [nb, 10] array into the world's BodyNodes through their
    setters (the device model is rebuilt on the next step)."""
    for i, (_, _, b, _, _) in enumerate(world._model_bodies()):
        if b is None:
            assert not P[i].any()
            continue
        b.setMass(float(P[i, 0]))
        b.setLocalCOM(P[i, 1:4])
        b.setMomentOfInertia(*[float(x) for x in P[i, 4:10]])
