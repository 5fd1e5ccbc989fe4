"""The backward's M-derivative field pairs two per pass (contact.cuh
mFieldsTerm; the default where the world inertias find a place on chip beside
the four fields: the dead Cholesky factor's, the pool's gRows / TAB slots or
the LDS pool area a world with its pool in the HBM workspace leaves idle,
which then also stages the NV columns) are the same operations in the same
order per element as one pair per pass (NIMBLE_AMD_BWD_MFUSE=0, read when the
device model is built), and the contact-free worlds' two Minv products in one
batched substitution are the two separate solves chain for chain
(NIMBLE_AMD_BWD_SOLVE2=0): gradients with and without must agree bit for bit,
in backpropState, in the wide (two rows per lane) backward and in the
Jacobian mode."""
import numpy as np
import pytest
import torch

from nimblephysics_amd import workloads
from test_gpu_contact_parity import SN_M, SN_NC, _device_backward, _device_step

pytestmark = pytest.mark.gpu

SN_IMP = 8          # csrc/pool_sizes.h: Q rank-deficient, four pairs instead of two
LDS_ROWS = 24       # csrc/capi.cpp ldsPoolRows: the most LCP rows an on-chip pool is sized for
WIDE_ROWS = 64      # csrc/capi.cpp deferRows: more rows take nimble_backward_wide_kernel
VARS = ("NIMBLE_AMD_BWD_MFUSE", "NIMBLE_AMD_BWD_SOLVE2")


def _rollout(make, B, var, on, monkeypatch, steps):
    monkeypatch.setenv(var, "1" if on else "0")
    try:
        world = make()
        world.setStatusPolicy("record")
        st, f = workloads.atlas_states(world, B, 1000)
        g = np.random.default_rng(11).standard_normal(st.shape)
        out, cache = [], None
        for _ in range(steps):
            nxt, snap, cache, ts, tf = _device_step(world, st, f, cache)
            gs, gf = _device_backward(world, ts, tf, snap, g)
            out.append((snap[:, :16].cpu().numpy(), nxt.cpu().numpy(), gs, gf))
            st = nxt.cpu().numpy()
    finally:
        monkeypatch.delenv(var, raising=False)
    return world, out


def _assert_same(on, off, tag):
    for step, (a, b) in enumerate(zip(on, off)):
        for name, x, y in zip(("snapshot header", "next state", "grad state", "grad action"), a, b):
            if name == "snapshot header":
                x, y = x[:, :SN_IMP + 1], y[:, :SN_IMP + 1]
            assert np.array_equal(x, y, equal_nan=True), (tag, step, name, np.flatnonzero(~np.all(x == y, axis=1))[:8])
        assert np.isfinite(a[2]).all() and np.isfinite(a[3]).all(), (tag, step)


@pytest.mark.parametrize("var", VARS)
def test_box_atlas_bit_identical(var, monkeypatch):
    """128 worlds of the bench's box-foot Atlas sampler (seed 1000), two
    chained steps.  The batch holds (step 1 / step 2) 15 / 14 clamping worlds
    with the imprecision flag (four pairs), 43 / 51 clamping worlds without
    it (two pairs) and 70 / 63 contact-free worlds (the batched plain solve);
    LCP rows 3..24, of which the backward's on-chip pool holds up to 11, so
    both the on-chip pool and the HBM workspace with the staged NV columns
    occur.  (Atlas has room for the inertias in the factor's place: every
    clamping world is fused, two passes / one pass in the stage-timing
    build's count.)"""
    world, on = _rollout(lambda: workloads.atlas_world(True), 128, var, True, monkeypatch, 2)
    _, off = _rollout(lambda: workloads.atlas_world(True), 128, var, False, monkeypatch, 2)
    for hd in (on[0][0], on[1][0]):
        m, nc, imp = hd[:, SN_M].astype(int), hd[:, SN_NC].astype(int), hd[:, SN_IMP] != 0
        print("clamping+imp", int(((nc > 0) & imp).sum()), "clamping", int(((nc > 0) & ~imp).sum()),
              "contact-free", int((nc == 0).sum()), "rows", np.unique(m).tolist())
        assert ((nc > 0) & imp).any()
        assert ((nc > 0) & ~imp).any()
        assert (nc == 0).any()
    _assert_same(on, off, var)


def test_mesh_atlas_bit_identical(monkeypatch):
    """64 worlds of the STL-mesh Atlas, one step: 11 clamping worlds have more
    than 64 LCP rows (nimble_backward_wide_kernel, R = 2) and 10 have 25-64
    (the one-row kernel with the pool in the HBM workspace): the pairs' fused
    pass with the NV columns copied into the idle LDS pool area, in both
    kernels."""
    var = VARS[0]
    world, on = _rollout(lambda: workloads.atlas_mesh_world(True), 64, var, True, monkeypatch, 1)
    _, off = _rollout(lambda: workloads.atlas_mesh_world(True), 64, var, False, monkeypatch, 1)
    hd = on[0][0]
    m, nc = hd[:, SN_M].astype(int), hd[:, SN_NC].astype(int)
    print("wide", int(((nc > 0) & (m > WIDE_ROWS)).sum()), "HBM pool", int(((nc > 0) & (m > LDS_ROWS) & (m <= WIDE_ROWS)).sum()))
    assert ((nc > 0) & (m > WIDE_ROWS)).any()
    assert ((nc > 0) & (m > LDS_ROWS) & (m <= WIDE_ROWS)).any()
    _assert_same(on, off, var)


def test_jacobian_mode_bit_identical(monkeypatch):
    """nimble_jacobians (2n items per world through backwardItems) on four
    contact worlds of the box-foot batch: the first two clamping worlds with
    the imprecision flag and the first two without it that have 12 or more
    LCP rows."""
    var = VARS[0]
    world = workloads.atlas_world(True)
    world.setStatusPolicy("record")
    st, f = workloads.atlas_states(world, 128, 1000)
    hd = _device_step(world, st, f)[1][:, :16].cpu().numpy()
    m, nc, imp = hd[:, SN_M].astype(int), hd[:, SN_NC].astype(int), hd[:, SN_IMP] != 0
    idx = np.concatenate([np.flatnonzero((nc > 0) & imp)[:2], np.flatnonzero((nc > 0) & ~imp & (m >= 12))[:2]])
    assert len(idx) == 4
    res = []
    for on in (True, False):
        monkeypatch.setenv(var, "1" if on else "0")
        try:
            w = workloads.atlas_world(True)
            w.setStatusPolicy("record")
            nxt, snap, cache, ts, tf = _device_step(w, st[idx], f[idx])
            J, F = w.native().jacobians(ts, tf, snap, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            res.append((snap[:, :16].cpu().numpy(), J.cpu().numpy(), F.cpu().numpy()))
        finally:
            monkeypatch.delenv(var, raising=False)
    assert np.array_equal(res[0][0][:, [SN_M, SN_NC, SN_IMP]], hd[idx][:, [SN_M, SN_NC, SN_IMP]])
    for name, x, y in zip(("snapshot header", "state Jacobian", "force Jacobian"), res[0], res[1]):
        if name == "snapshot header":
            x, y = x[:, :SN_IMP + 1], y[:, :SN_IMP + 1]
        assert np.array_equal(x, y, equal_nan=True), name
    assert np.isfinite(res[0][1]).all() and np.abs(res[0][1]).max() > 0
