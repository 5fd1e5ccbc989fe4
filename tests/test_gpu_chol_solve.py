"""The solves with the mass matrix's Cholesky factor (csrc/chol_wave.cuh) give
the bits they gave before they were restructured into straight-line, blocked
code: nimble.timestep forward + backward on the cases of chol_solve_cases.py
(cartpole n = 2, KR5 with the ground skeleton n = 6, box-foot Atlas n = 33 over
two warm-started steps) against tests/golden/chol_solve_parent.npz, recorded
on the GPU with the library of the commit before the change
(tools/gen_chol_solve_golden.py).  Bit for bit, through int64 views.

The Atlas batch must hold at least two clamping worlds (the backward's batched
solves of 5 and 4 columns) and two contact-free ones (the two-column solve) in
each step, as it did when recorded: 4 and 4 in both.

NIMBLE_AMD_BWD_SOLVE2=0 (the contact-free worlds' two single-column solves
instead of the two-column one) must give the default's bits.
"""
import os

import numpy as np
import pytest

import chol_solve_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chol_solve_parent.npz")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def atlas_default():
    world, st, f, steps = cases.cases()["atlas"]
    return cases.run(world, st, f, steps)


def _check(name, res, golden):
    keys = [k for k in golden.files if k.startswith(name + "/")]
    assert len(keys) == len(res) and keys
    for k in keys:
        got, want = res[k.split("/", 1)[1]], golden[k]
        assert got.shape == want.shape, k
        same = np.array_equal(_bits(got), _bits(want))
        if not same:
            bad = np.argwhere(_bits(got) != _bits(want))
            print(k, "differs at", bad[:8].tolist(), "max abs diff", np.abs(got - want).max())
        assert same, k


@pytest.mark.parametrize("name", ["cartpole", "kr5_ground"])
def test_small_models_bits(name, golden):
    world, st, f, steps = cases.cases()[name]
    _check(name, cases.run(world, st, f, steps), golden)


def test_atlas_bits(atlas_default, golden):
    counts = cases.atlas_counts(atlas_default)
    print("atlas (clamping, contact-free) per step:", counts)
    for clamping, free in counts:
        assert clamping >= cases.MIN_WORLDS and free >= cases.MIN_WORLDS, counts
    _check("atlas", atlas_default, golden)


def test_atlas_single_column_solves_same_bits(atlas_default, monkeypatch):
    monkeypatch.setenv("NIMBLE_AMD_BWD_SOLVE2", "0")
    try:
        world, st, f, steps = cases.cases()["atlas"]
        res = cases.run(world, st, f, steps)
    finally:
        monkeypatch.delenv("NIMBLE_AMD_BWD_SOLVE2", raising=False)
    for clamping, free in cases.atlas_counts(res):
        assert free >= cases.MIN_WORLDS
    assert sorted(res) == sorted(atlas_default)
    for k in res:
        assert np.array_equal(_bits(res[k]), _bits(atlas_default[k])), k
