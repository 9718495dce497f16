"""Pose scoring on the device (icpk_score_poses, K15): partners against the existing exact NN path, sums and counts
against the numpy model of the rule (tests/score_model.py), bit for bit; the context's state untouched; argument
errors; SequenceRunner's score_max_dist."""
import ctypes as C

import numpy as np
import pytest

import gicp_model as gm
import score_model as sm
import tsdf_cases
from icp_slam_prototype_amd import binding, sequence, synth

pytestmark = pytest.mark.gpu


def pose(rx=0.0, ry=0.0, rz=0.0, t=(0.0, 0.0, 0.0), about=(5.0, 5.0, 5.0)):
    """row-major 4 x 4 float32: a rotation about `about` followed by a translation"""
    R = synth.rot_xyz_deg(rx, ry, rz)
    c = np.asarray(about, np.float64)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = c - R @ c + np.asarray(t, np.float64)
    return T.astype(np.float32)


def clouds(ns, nt, seed, dup=0.0):
    """A target of nt points and a source whose points lie at every scale of distance from it: on a target point,
    millimetres, centimetres and decimetres off, and metres away (the walk ends in its first round, after a find
    beyond the radius, after doublings, or without a partner)."""
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(4.0, 6.0, (3, nt)).astype(np.float32)
    if dup > 0 and nt > 1:
        k = int(dup * nt)
        at = rng.choice(nt, k, replace=False)
        tgt[:, at] = tgt[:, rng.integers(0, nt, k)]  # exact duplicates, at lower and higher indices
    base = tgt[:, rng.integers(0, nt, ns)].astype(np.float64)
    scale = np.array([0.0, 1e-3, 2e-2, 0.3, 3.0])[rng.integers(0, 5, ns)]
    src = base + rng.normal(0, 1, (3, ns)) * scale
    return src.astype(np.float32), tgt


def check_model(src, tgt, T, max_dist, keep=True):
    """score_poses against the model for every pose: sums, inliers and (keep) partners, bit for bit"""
    T = np.asarray(T, np.float32).reshape(-1, 4, 4)
    with binding.Context(0) as c:
        c.set_target(tgt)
        c.set_source(src)
        out = c.score_poses(T, max_dist, keep_assoc=keep)
        assoc = [c.score_associations(k) for k in range(len(T))] if keep else None
    assert out["sums"].shape == (len(T), 11) and out["information"].shape == (len(T), 6, 6)
    for k in range(len(T)):
        want = sm.score(src, tgt, T[k], max_dist)
        assert out["inliers"][k] == want["inliers"], (k, out["inliers"][k], want["inliers"])
        assert out["sums"][k].tobytes() == want["sums"].tobytes(), (k, out["sums"][k], want["sums"])
        if keep:
            assert np.array_equal(assoc[k][0], want["idx"]), k
            assert assoc[k][1].tobytes() == want["dist"].tobytes(), k
        met = sm.metrics(want["sums"], want["inliers"], src.shape[1])
        assert (out["fitness"][k], out["inlier_rmse"][k], out["mean_dist"][k]) == met
        assert out["information"][k].tobytes() == sm.information(want["sums"], want["inliers"]).tobytes()
    return out


SMALL = [pose(), pose(0.3, -0.5, 0.2, (0.004, -0.003, 0.002))]


@pytest.fixture(scope="module")
def quarter():
    return gm.quarter_pair()


def test_partners_equal_the_exact_nn_path_and_the_context_is_untouched(quarter):
    src, tgt = quarter["source"], quarter["target"]
    max_dist = 0.05
    T = np.stack([pose(), pose(0, 2.0, 0, (0.03, 0, 0)), pose(0.5, -1.0, 0.3, (-0.02, 0.01, 0.0)),
                  pose(-1.5, 0.2, 1.0, (0.0, 0.05, -0.04)), pose(t=(100.0, -80.0, 60.0))])
    with binding.Context(0) as c, binding.Context(0) as never, binding.Context(0) as ref:
        for x in (c, never, ref):
            x.set_target(tgt)
            x.set_source(src)
        for x in (c, never):  # a state to be left alone: a moved working source and the associations of a sweep
            x.transform_source(T[1][:3, :3], T[1][:3, 3])
            x.nn(binding.NN_GRID, fetch=False)
        out = c.score_poses(T, max_dist, keep_assoc=True)
        for k in range(len(T)):
            ref.reset_source()
            ref.transform_source(T[k][:3, :3], T[k][:3, 3])
            idx, dist = ref.nn(binding.NN_EXACT)
            si, sd = c.score_associations(k)
            acc = dist < np.float32(max_dist)
            assert np.array_equal(si[acc], idx[acc]) and sd[acc].tobytes() == dist[acc].tobytes(), k
            assert (si[~acc] == -1).all() and np.isposinf(sd[~acc]).all(), k
            assert out["inliers"][k] == acc.sum(), k
        assert out["inliers"][4] == 0 and 0 < out["inliers"][0] < src.shape[1]
        assert c.get_source().tobytes() == never.get_source().tobytes()
        a, b = c.get_associations(), never.get_associations()
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()
        ra = c.align(solve=binding.SOLVE_KABSCH, max_iterations=5, fixed_iterations=1)
        rb = never.align(solve=binding.SOLVE_KABSCH, max_iterations=5, fixed_iterations=1)
        assert ra[0].tobytes() == rb[0].tobytes() and ra[2] == rb[2]
        assert bytes(ra[1]) == bytes(rb[1])
        assert c.get_source().tobytes() == never.get_source().tobytes()


@pytest.mark.parametrize("ns", [1, 255, 257, 65536 + 300])
def test_model_source_sizes(ns):
    src, tgt = clouds(ns, 300, seed=ns)
    check_model(src, tgt, SMALL, 0.1)


@pytest.mark.parametrize("nt", [1, 7])
def test_model_one_cell_targets(nt):
    src, tgt = clouds(257, nt, seed=20 + nt)
    check_model(src, tgt, SMALL, 0.75)


def test_model_duplicate_targets_tie_to_the_lowest_index():
    src, tgt = clouds(300, 500, seed=31, dup=0.4)
    out = check_model(src, tgt, SMALL, 0.1)
    idx = sm.score(src, tgt, SMALL[0], 0.1)["idx"]
    dup_hits = [j for j in idx[idx >= 0] if (tgt == tgt[:, [j]]).all(0).sum() > 1]
    assert len(dup_hits) > 5 and out["inliers"][0] > 100  # (the ties are really there)
    for j in dup_hits:
        assert j == np.flatnonzero((tgt == tgt[:, [j]]).all(0))[0]


@pytest.mark.parametrize("max_dist", [1e-3, 0.1, 0.75, 50.0])
def test_model_max_dist(max_dist):
    src, tgt = clouds(500, 2000, seed=41)
    out = check_model(src, tgt, SMALL + [pose(t=(0.0, 1.5, 0.0))], max_dist)
    if max_dist == 50.0:
        assert (out["inliers"] == 500).all()


@pytest.mark.parametrize("n_poses,ns", [(1, 400), (2, 400), (17, 400), (300, 2000)])
def test_model_pose_counts(n_poses, ns):
    rng = np.random.default_rng(50 + n_poses)
    src, tgt = clouds(ns, 300, seed=51)
    T = [pose(*rng.normal(0, 0.5, 3), rng.normal(0, 0.01, 3)) for _ in range(n_poses)]
    for k in range(3, n_poses, 4):  # a quarter far off
        T[k] = pose(*rng.normal(0, 20, 3), rng.normal(0, 1.0, 3))
    check_model(src, tgt, T, 0.1, keep=n_poses <= 17)


def test_model_nan_pose_and_non_finite_targets():
    src, tgt = clouds(300, 400, seed=61)
    bad = pose(0.2, 0.1, 0.0)
    bad[1, 2] = np.nan
    out = check_model(src, tgt, [SMALL[1], bad, SMALL[0]], 0.1)
    assert out["inliers"][1] == 0 and out["inliers"][0] > 0 and out["inliers"][2] > 0
    tgt2 = tgt.copy()
    tgt2[0, 5], tgt2[1, 100], tgt2[:, 399] = np.nan, np.inf, -np.inf
    src2 = src.copy()
    src2[2, 7] = np.nan
    check_model(src2, tgt2, SMALL, 0.1)


def test_partner_does_not_depend_on_the_order_of_the_target():
    src, tgt = clouds(600, 1500, seed=71)
    perm = np.random.default_rng(72).permutation(tgt.shape[1])
    res = []
    for t in (tgt, tgt[:, perm]):
        with binding.Context(0) as c:
            c.set_target(t)
            c.set_source(src)
            out = c.score_poses(SMALL, 0.1, keep_assoc=True)
            idx, d = c.score_associations(1)
        res.append((out["inliers"].copy(), d, np.where(idx >= 0, t[:, np.maximum(idx, 0)], np.float32(0))))
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1].tobytes() == res[1][1].tobytes()
    assert res[0][2].tobytes() == res[1][2].tobytes()


def test_scoring_the_working_source_after_an_alignment(quarter):
    max_dist = 0.3
    with binding.Context(0) as c:
        c.set_target(quarter["target"])
        c.set_source(quarter["source"])
        T, st, rc = c.align(solve=binding.SOLVE_KABSCH, max_iterations=5, fixed_iterations=1, max_nn_dist=max_dist)
        assert rc == 0
        out = c.score_poses(None, max_dist, keep_assoc=True)
        assert out["inliers"][0] == st.final_pairs
        si, sd = c.score_associations(0)
        idx, dist = c.get_associations()
        acc = dist < np.float32(max_dist)
        assert acc.sum() == st.final_pairs
        assert np.array_equal(si[acc], idx[acc]) and sd[acc].tobytes() == dist[acc].tobytes()
        assert (si[~acc] == -1).all() and np.isposinf(sd[~acc]).all()
        assert 0 < out["fitness"][0] <= 1 and out["inlier_rmse"][0] >= out["mean_dist"][0] > 0


def test_the_same_call_three_times_gives_the_same_bytes():
    src, tgt = clouds(3000, 3000, seed=81)
    T = SMALL + [pose(1.0, 1.0, 1.0, (0.05, 0.0, 0.0))]
    got = []
    with binding.Context(0) as c:
        c.set_target(tgt)
        c.set_source(src)
        for _ in range(3):
            out = c.score_poses(T, 0.1, keep_assoc=True)
            a = [c.score_associations(k) for k in range(3)]
            got.append(out["sums"].tobytes() + out["inliers"].tobytes() + b"".join(i.tobytes() + d.tobytes() for i, d in a))
    assert got[0] == got[1] == got[2]


def raw_score(c, n, T, max_dist, flags=0, sums=True, inliers=True):
    s = np.zeros((max(n, 1), 11), np.float64)
    i = np.zeros(max(n, 1), np.int64)
    Tf = None if T is None else np.ascontiguousarray(T, np.float32)
    rc = c._lib.icpk_score_poses(c._h, n, None if Tf is None else binding._fp(Tf), max_dist, flags,
                                 s.ctypes.data_as(C.POINTER(C.c_double)) if sums else None,
                                 i.ctypes.data_as(C.POINTER(C.c_int64)) if inliers else None)
    return rc, s, i


def test_argument_errors():
    src, tgt = clouds(200, 300, seed=91)
    T = np.stack(SMALL)
    many = np.tile(pose(), (binding.SCORE_MAX_POSES + 1, 1, 1))
    with binding.Context(0) as c:
        assert raw_score(c, 1, T[:1], 0.1)[0] == binding.E_NOT_SET
        c.set_target(tgt)
        assert raw_score(c, 1, T[:1], 0.1)[0] == binding.E_NOT_SET
        with pytest.raises(binding.IcpkError) as e:
            c.score_associations(0)
        assert e.value.code == binding.E_NOT_SET
        c.set_source(src)
        c.score_poses(T, 0.1)  # (without the flag nothing is kept)
        with pytest.raises(binding.IcpkError) as e:
            c.score_associations(0)
        assert e.value.code == binding.E_NOT_SET
        c.score_poses(T, 0.1, keep_assoc=True)
        kept = c.score_associations(1)

        def still_there():
            a = c.score_associations(1)
            return np.array_equal(a[0], kept[0]) and a[1].tobytes() == kept[1].tobytes()

        bad = [raw_score(c, 0, T, 0.1), raw_score(c, -1, T, 0.1), raw_score(c, binding.SCORE_MAX_POSES + 1, many, 0.1),
               raw_score(c, 2, None, 0.1), raw_score(c, 0, None, 0.1), raw_score(c, 2, T, 0.0), raw_score(c, 2, T, -1.0),
               raw_score(c, 2, T, float("nan")), raw_score(c, 2, T, float("inf")), raw_score(c, 2, T, 0.1, flags=2),
               raw_score(c, 2, T, 0.1, flags=-1), raw_score(c, 2, T, 0.1, sums=False),
               raw_score(c, 2, T, 0.1, inliers=False)]
        for k, (rc, s, i) in enumerate(bad):
            assert rc == binding.E_ARG and not s.any() and not i.any(), k
            assert still_there(), k
        assert c._lib.icpk_score_poses(None, 1, None, 0.1, 0, None, None) == binding.E_ARG
        for p in (-1, 2, 1 << 20):
            with pytest.raises(binding.IcpkError) as e:
                c.score_associations(p)
            assert e.value.code == binding.E_ARG
        assert raw_score(c, binding.SCORE_MAX_POSES, many[:-1], 0.1)[0] == binding.OK  # the largest call there is
        c.score_poses(T[:1], 0.1)  # a later call without the flag leaves the kept associations as they are
        assert still_there()
        # an empty target: what icpk_nn returns for it
        with binding.Context(0) as e2:
            e2.set_target(np.zeros((3, 0), np.float32))
            e2.set_source(src)
            want = e2._lib.icpk_nn(e2._h, binding.NN_EXACT, None, None)
            assert want < 0 and raw_score(e2, 1, T[:1], 0.1)[0] == want
        # an empty source: zero sums, zero inliers
        with binding.Context(0) as e3:
            e3.set_target(tgt)
            e3.set_source(np.zeros((3, 0), np.float32))
            out = e3.score_poses(T, 0.1, keep_assoc=True)
            assert not out["sums"].any() and not out["inliers"].any() and not out["fitness"].any()
            assert e3.score_associations(1)[0].size == 0
        # the kept associations belong to the clouds they were scored on
        c.set_source(src)
        with pytest.raises(binding.IcpkError) as e:
            c.score_associations(0)
        assert e.value.code == binding.E_NOT_SET
        c.score_poses(T, 0.1, keep_assoc=True)
        assert still_there()
        c.set_target(tgt)
        with pytest.raises(binding.IcpkError) as e:
            c.score_associations(0)
        assert e.value.code == binding.E_NOT_SET
        # ... and a TSDF hand-over is a new target (with and without ICPK_TSDF_COLOR)
        for raycast in (False, True):
            for color in (False, True):
                c.set_target(tgt)
                c.score_poses(T, 0.1, keep_assoc=True)
                assert still_there()
                tsdf_cases.hand_over(c, raycast=raycast, color=color)
                with pytest.raises(binding.IcpkError) as e:
                    c.score_associations(0)
                assert e.value.code == binding.E_NOT_SET, (raycast, color)
        c.tsdf_release()


def test_sequence_runner_reports_fitness_when_asked():
    rows, cols = 96, 128
    rng = np.random.default_rng(5)
    frames = []
    for k in range(4):
        d = synth.render_room_depth(rows, cols, synth.rot_xyz_deg(0, 0.4 * k, 0.1 * k), np.array([0.008 * k, 0, 0]),
                                    noise_sigma=0.001, rng=rng)
        d[rng.random(d.shape) > 0.6] = 0
        frames.append(d.astype(np.uint16))
    with binding.Context(0) as a, binding.Context(0) as b:
        scored = sequence.SequenceRunner(a, max_iterations=6, threshold=1e-6, score_max_dist=0.1)
        plain = sequence.SequenceRunner(b, max_iterations=6, threshold=1e-6)

        def forbidden(*args, **kw):
            raise AssertionError("score_poses called without score_max_dist")

        b.score_poses = forbidden
        oa = [scored.step(f) for f in frames]
        ob = [plain.step(f) for f in frames]
    assert oa[0] is None and ob[0] is None
    for ra, rb in zip(oa[1:], ob[1:]):
        assert 0 < ra["fitness"] <= 1 and ra["inlier_rmse"] > 0
        assert set(ra) - set(rb) == {"fitness", "inlier_rmse"} and set(rb) <= set(ra)
        for key, v in rb.items():
            assert np.array_equal(np.asarray(ra[key]), np.asarray(v)), key
