"""bench.py's plain run and its options: --steps sets the timed steps, the
plain line carries the headline keys and nothing that takes a run of its own
(that is behind --full), and --dump-outputs DIR writes what the last timed
step returned -- next state, state and action gradients -- as DIR/<name>.npy,
identical from run to run.  On the CPU the oracle stands in for the GPU
timestep (as in test_host's launcher tests); the -m gpu test runs the product
path."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import models
from test_host import _BOX_WL, _OracleTimestep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
NAMES = ("next_state", "grad_state", "grad_action")


def _load(d):
    return {k: np.load(os.path.join(d, k + ".npy")) for k in NAMES}


def test_full_is_off_by_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert a.full is False and a.dump_outputs is None
    assert bench.parse_args(["--full"]).full is True


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    last = {"next_state": torch.arange(400, dtype=torch.float64).reshape(100, 4),
            "grad_state": torch.ones(100, 4, dtype=torch.float64),
            "grad_action": torch.ones(100, 2, dtype=torch.float64)}
    bench.dump_outputs(last, str(tmp_path / "all"), 0)
    got = _load(tmp_path / "all")
    assert all(got[k].dtype == np.float64 for k in NAMES)
    assert np.array_equal(got["next_state"], last["next_state"].numpy())
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1000)
    bench.dump_outputs(last, str(tmp_path / "a"), 0)
    bench.dump_outputs(last, str(tmp_path / "b"), 0)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(v.nbytes for v in a.values()) <= 1000
    assert 0 < len(a["next_state"]) < 100
    for k in NAMES:
        assert np.array_equal(a[k], b[k])
    # rows of the full array, in order
    rows = (a["next_state"][:, 0] / 4).astype(int)
    assert np.array_equal(a["next_state"], last["next_state"].numpy()[rows]) and (np.diff(rows) > 0).all()


def test_plain_cpu_run_dumps_last_step(oracle_built, tmp_path, monkeypatch):
    """`--device cpu` run of the box workload with the oracle timestep: the
    dumped arrays are those of timed step `steps` of the rollout (warmup
    included), and a second run writes the same bytes."""
    from oracle.oracle import OracleWorld
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setitem(bench.WORKLOADS, "box", _BOX_WL)
    ows = {}

    def ts(w, s, a):
        return _OracleTimestep.apply(ows.setdefault(id(w), OracleWorld(w)), w, s, a)

    monkeypatch.setattr(bench, "nimble", SimpleNamespace(timestep=ts))
    runs = []
    for name in ("a", "b"):
        out = tmp_path / f"{name}.json"
        bench.main(["--gpus", "1", "--device", "cpu", "--workload", "box", "--steps", "2", "--warmup", "1",
                    "--dump-outputs", str(tmp_path / name), "--out", str(out)])
        line = json.loads(out.read_text())
        assert all(k in line for k in HEADLINE_KEYS) and line["steps"] == 2 and line["ms_per_step"] > 0
        assert abs(line["value"] - 6 / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
        for k in ("cpu_baseline", "atlas_mesh", "roofline"):
            assert k not in line
        runs.append(_load(tmp_path / name))
    for k in NAMES:
        assert runs[0][k].dtype == np.float64 and np.array_equal(runs[0][k], runs[1][k])
    # the third step of the rollout, recomputed here
    world = models.box_world()
    ow = OracleWorld(world)
    st, f, g = bench.rank_inputs(world, models._box_sampler, 6, 0)
    state, action, g = torch.from_numpy(st), torch.from_numpy(f), torch.from_numpy(g)
    for _ in range(3):
        s, a = state.detach().requires_grad_(True), action.detach().requires_grad_(True)
        nxt = _OracleTimestep.apply(ow, world, s, a)
        nxt.backward(g)
        state = nxt.detach()
    assert np.array_equal(runs[0]["next_state"], state.numpy())
    assert np.array_equal(runs[0]["grad_state"], s.grad.numpy())
    assert np.array_equal(runs[0]["grad_action"], a.grad.numpy())


@pytest.mark.gpu
def test_plain_gpu_run_dumps_last_step(tmp_path):
    """The product path: a plain run of 64 Atlas-on-ground worlds writes the
    headline line without the --full objects, counts exactly --steps timed
    steps, and dumps the outputs of the rollout's last step, which equal a
    rollout of nimble.timestep made here from the same seeded inputs."""
    import nimblephysics_amd as nimble
    counted = []
    step0 = bench.nimble.timestep

    def counting(w, s, a):
        counted.append(1)
        return step0(w, s, a)

    bench.nimble = SimpleNamespace(timestep=counting)
    try:
        out = tmp_path / "bench.json"
        bench.run(bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "64",
                                    "--dump-outputs", str(tmp_path / "dump"), "--out", str(out)]))
    finally:
        bench.nimble = nimble
    assert len(counted) == 5  # 2 warmup + 3 timed steps, nothing replayed
    line = json.loads(out.read_text())
    assert all(k in line for k in HEADLINE_KEYS) and line["steps"] == 3 and line["dtype"] == "f64"
    assert abs(line["value"] - 64 / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    for k in ("cpu_baseline", "atlas_mesh", "roofline"):
        assert k not in line
    got = _load(tmp_path / "dump")
    world = models.atlas_world(with_ground=True)
    st, f, g = bench.rank_inputs(world, bench.WORKLOADS["atlas"][2], 64, 0)
    state = torch.tensor(st, device="cuda:0")
    action, g = torch.tensor(f, device="cuda:0"), torch.tensor(g, device="cuda:0")
    for _ in range(5):
        s, a = state.detach().requires_grad_(True), action.detach().requires_grad_(True)
        nxt = nimble.timestep(world, s, a)
        nxt.backward(g)
        state = nxt.detach()
    assert got["next_state"].shape == (64, 66) and got["next_state"].dtype == np.float64
    assert np.isfinite(got["next_state"]).all() and np.abs(got["grad_state"]).sum() > 0
    assert np.array_equal(got["next_state"], state.cpu().numpy())
    assert np.array_equal(got["grad_state"], s.grad.cpu().numpy())
    assert np.array_equal(got["grad_action"], a.grad.cpu().numpy())
