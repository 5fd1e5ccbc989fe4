"""cholSolveReg<K> (csrc/chol_wave.cuh) on the CPU: the straight-line, blocked
substitution compiled for the host with AddressSanitizer against the emulated
wavefront (tests/cpp/wave_emu/chol_solve_emu.cpp) and compared bit for bit,
through int64 views, with the plain scalar substitution it replaces (k
ascending: x_k <- x_k dinv_k, x_i <- fma(-L_ik, x_k, x_i) for i > k; then the
mirror image), which the driver runs next to it.

Shapes: n in {0, 1, 2, 7, 8, 9, 16, 33, 63, 64} (nothing to do, no full block
of eight steps, exactly one, one plus a tail, the Atlas size, the full wave)
times K in {1, 2, 4, 5} right-hand sides.  The factor is that of a
well-conditioned random matrix, stored between NaN guards; the right-hand
sides hold +0.0, -0.0 and subnormals among ordinary values; lanes >= n carry
sentinels that must come back untouched.  A second set makes one column's
right-hand side inf at one row: the other K - 1 columns must still match the
reference bit for bit (the inf column itself up to which NaN it holds).

All cases run in one process, once per session.  No GPU needed.
"""
import os
import subprocess

import numpy as np
import pytest

import wave_emu

pytestmark = pytest.mark.skipif(not os.path.exists(wave_emu.CLANG), reason="needs the ROCm clang for the host build")

NS = (0, 1, 2, 7, 8, 9, 16, 33, 63, 64)
KS = (1, 2, 4, 5)
CASES = [(n, K, inf) for inf in (False, True) for n in NS for K in KS if not (inf and n == 0)]


def _inputs(n, K, inf):
    """packed factor, dinv, x [K, 64] and the (column, row) made inf (or None)"""
    rng = np.random.default_rng(1000 * n + 10 * K + int(inf))
    A = rng.standard_normal((n, n))
    L = np.linalg.cholesky(A @ A.T + n * np.eye(n)) if n else np.zeros((0, 0))
    packed = np.array([L[i, k] for i in range(n) for k in range(i + 1)])
    dinv = 1.0 / np.diag(L) if n else np.zeros(0)
    x = rng.standard_normal((K, 64))
    # special values among the right-hand sides (rows that exist)
    specials = [0.0, -0.0, 5e-324, -5e-324, 2.2e-308 / 4, -1e-310]
    for q in range(K):
        for j, v in enumerate(specials):
            if n:
                x[q, (3 * q + 5 * j) % n] = v
    x[:, n:] = 1000.0 + np.arange(K)[:, None] + np.arange(64 - n)[None, :] / 64.0  # sentinels
    hit = None
    if inf:
        hit = (K - 1, n // 2)
        x[hit] = np.inf
    return packed, dinv, x, hit


@pytest.fixture(scope="module")
def results():
    exe = wave_emu.build("chol_solve_emu")
    f = wave_emu._fmt
    lines = [str(len(CASES))]
    for n, K, inf in CASES:
        packed, dinv, x, _ = _inputs(n, K, inf)
        lines += [f"{n} {K}", f(packed), f(dinv), f(x)]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], input="\n".join(lines), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    out = r.stdout.splitlines()
    assert len(out) == 2 * len(CASES)
    res = {}
    for c, case in enumerate(CASES):
        new, ref = out[2 * c].split(), out[2 * c + 1].split()
        assert new[0] == "new" and ref[0] == "ref"
        K = case[1]
        res[case] = (np.array(new[1:], dtype=np.int64).reshape(K, 64),
                     np.array(ref[1:], dtype=np.int64).reshape(K, 64))
    return res


@pytest.mark.parametrize("n,K,inf", CASES)
def test_chol_solve_bits(results, n, K, inf):
    new, ref = results[(n, K, inf)]
    packed, dinv, x, hit = _inputs(n, K, inf)
    # lanes >= n: the inputs, bit for bit (the reference never touches them)
    assert np.array_equal(new[:, n:], x[:, n:].view(np.int64))
    assert np.array_equal(ref[:, n:], x[:, n:].view(np.int64))
    cols = [q for q in range(K) if hit is None or q != hit[0]]
    assert np.array_equal(new[cols], ref[cols])
    got = new.view(np.float64)
    if hit is not None:
        a, b = got[hit[0]], ref.view(np.float64)[hit[0]]
        assert np.array_equal(np.isnan(a), np.isnan(b))
        ok = ~np.isnan(a)
        assert np.array_equal(new[hit[0]][ok], ref[hit[0]][ok])
        assert not np.isfinite(a[:n]).all()
    # no NaN guard reached a finite column, and the reference is a solve:
    # L L^T x = b to rounding
    assert np.isfinite(got[cols]).all()
    if n:
        L = np.zeros((n, n))
        L[np.tril_indices(n)] = packed
        for q in cols:
            r = L @ (L.T @ got[q, :n]) - x[q, :n]
            assert np.abs(r).max() <= 1e-12 * (1.0 + np.abs(x[q, :n]).max())
