"""Pose scoring (icpk_score_poses, K15) without a device: the numpy model of the rule (tests/score_model.py) against an
explicitly formed information matrix, and the library's two host functions (icpk_score_metrics,
icpk_information_matrix) against the model, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import score_model as sm
from icp_slam_prototype_amd import binding, build


@pytest.fixture(scope="module")
def lib():
    build.build()
    return binding.load()


def _cloud(rng, n):
    return (rng.normal(0, 1.5, (3, n)) + np.array([[5.0], [5.0], [7.0]])).astype(np.float32)


def test_model_information_equals_explicit_sum():
    """sum G^T G assembled from the eleven sums against the same matrix formed point by point in float64.  Both are
    sums of n products of magnitude <= |q|^2, each addition rounding by 2^-53 of the running sum: the difference is
    bounded by n 2^-53 of the Frobenius norm, 1.1e-11 for n = 10^5; 1e-9 leaves two to three orders of margin."""
    rng = np.random.default_rng(11)
    for n in (1, 7, 1000, 100000):
        tgt = _cloud(rng, n)
        idx = np.arange(n, dtype=np.int32)
        dist = np.zeros(n, np.float32)
        sums = sm.canonical(sm.terms(tgt, idx, dist))
        got = sm.information(sums, n)
        if n <= 1000:
            want = sm.information_explicit(tgt)
        else:  # the same sum without a Python loop over 10^5 points
            q = tgt.astype(np.float64)
            G = np.zeros((n, 3, 6))
            G[:, 0, 1], G[:, 0, 2] = q[2], -q[1]
            G[:, 1, 0], G[:, 1, 2] = -q[2], q[0]
            G[:, 2, 0], G[:, 2, 1] = q[1], -q[0]
            G[:, 0, 3] = G[:, 1, 4] = G[:, 2, 5] = 1.0
            want = np.einsum("kia,kib->ab", G, G)
        assert np.linalg.norm(got - want) <= 1e-9 * np.linalg.norm(want), n


def test_information_matrix_is_symmetric_and_psd():
    rng = np.random.default_rng(12)
    tgt = _cloud(rng, 500)
    idx = np.where(rng.random(500) < 0.7, np.arange(500), -1).astype(np.int32)
    dist = rng.uniform(0, 0.1, 500).astype(np.float32)
    sums = sm.canonical(sm.terms(tgt, idx, dist))
    n = int((idx >= 0).sum())
    for info in (sm.information(sums, n), binding.information_matrix(sums, n)):
        assert np.array_equal(info, info.T)
        w = np.linalg.eigvalsh(info)
        assert w.min() > 0 and w.min() > -1e-12 * w.max()  # a cloud that is no line and no point: positive definite
        assert np.array_equal(np.diag(info)[3:], [n, n, n])


def test_host_functions_equal_the_model_bit_for_bit(lib):
    rng = np.random.default_rng(13)
    cases = []
    for _ in range(200):
        s = rng.normal(0, 1, sm.NSCORE) * 10.0 ** rng.uniform(-3, 6, sm.NSCORE)
        s[[0, 1, 5, 8, 10]] = np.abs(s[[0, 1, 5, 8, 10]])
        cases.append((s, int(rng.integers(1, 1 << 20)), int(rng.integers(1, 1 << 20))))
    cases.append((np.zeros(sm.NSCORE), 0, 1000))       # no inliers
    cases.append((np.zeros(sm.NSCORE), 0, 0))          # no source
    cases.append((rng.normal(0, 1, sm.NSCORE) ** 2, 5, 0))
    cases.append((np.ones(sm.NSCORE), 1, 1))
    for s, inl, ns in cases:
        got = binding.score_metrics(s, inl, ns)
        want = sm.metrics(s, inl, ns)
        assert np.array(got, np.float32).tobytes() == np.array(want, np.float32).tobytes(), (s, inl, ns)
        assert binding.information_matrix(s, inl).tobytes() == sm.information(s, inl).tobytes(), (s, inl)
    assert binding.score_metrics(np.zeros(sm.NSCORE), 0, 0) == (0, 0, 0)


def test_host_functions_by_raw_ctypes(lib):
    """a struct-free call of the two new host symbols (tests/test_abi.py checks that the header's symbols are exported)"""
    dp = C.POINTER(C.c_double)
    sums = np.arange(1, 12, dtype=np.float64)
    f, r, m = C.c_float(-1), C.c_float(-1), C.c_float(-1)
    lib.icpk_score_metrics(sums.ctypes.data_as(dp), 4, 8, C.byref(f), C.byref(r), C.byref(m))
    assert (f.value, r.value, m.value) == (0.5, np.float32(np.sqrt(0.5)), 0.25)
    lib.icpk_score_metrics(sums.ctypes.data_as(dp), 4, 8, None, None, None)  # every output may be NULL
    info = np.full(36, np.nan)
    lib.icpk_information_matrix(sums.ctypes.data_as(dp), 4, info.ctypes.data_as(dp))
    info = info.reshape(6, 6)
    assert info[0, 0] == 9 + 11 and info[1, 1] == 6 + 11 and info[2, 2] == 6 + 9
    assert (info[0, 1], info[0, 2], info[1, 2]) == (-7, -8, -10)
    assert np.array_equal(info[:3, 3:], [[0, -5, 4], [5, 0, -3], [-4, 3, 0]]) and np.array_equal(info[3:, 3:], 4 * np.eye(3))
    assert np.array_equal(info, info.T)
    assert (binding.NSCORE, binding.SCORE_MAX_POSES, binding.SCORE_KEEP_ASSOC) == (11, 4096, 1)


def test_model_transform_and_partners_equal_the_oracle(oracle):
    """the model's two geometric steps against the oracle's restatement of the reference (transform_points,
    nn_bruteforce): the same bits, and the same partner wherever it lies within max_dist"""
    rng = np.random.default_rng(14)
    tgt = _cloud(rng, 700)
    src = (tgt[:, rng.integers(0, 700, 400)] + rng.normal(0, 0.05, (3, 400))).astype(np.float32)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = binding.make_rotation_matrix(1.0, -2.0, 0.5)
    T[:3, 3] = [0.01, -0.02, 0.03]
    p = sm.transform(src, T)
    assert p.tobytes() == oracle.transform_points(src, T[:3, :3].copy(), T[:3, 3].copy()).tobytes()
    oidx, odist = oracle.nn_bruteforce(p, tgt, threads=2)
    idx, dist = sm.partners(p, tgt, 0.3)
    acc = odist < np.float32(0.3)
    assert 0 < acc.sum() < 400, acc.sum()
    assert np.array_equal(idx[acc], oidx[acc]) and dist[acc].tobytes() == odist[acc].tobytes()
    assert (idx[~acc] == -1).all() and np.isposinf(dist[~acc]).all()
