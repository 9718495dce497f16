"""RANSAC plane segmentation (K34) without a GPU: the numpy model of THE PLANE RULE (tests/plane_model.py), a literal
triple loop in scalar arithmetic, and the library's host-only icpk_segment_planes_host against one another, bit for bit;
what the rule promises on constructed clouds; the refit against numpy.linalg.eigh; the refusals of the host functions; and
what the segmentation finds in config 2's target (model = host function)."""
import ctypes as C

import numpy as np
import pytest

import plane_model as pm
from icp_slam_prototype_amd import binding, build, planes, synth

LOOP_MAX = 700  # points up to which the Python triple loop runs in a moment


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()


def _three(pts, **kw):
    """the model's record, held to the host function's and (small clouds) the triple loop's"""
    want = pm.segment(pts, **kw)
    host = planes.segment_host(pts, **kw)
    assert pm.same(host, want) is None, ("host", pm.same(host, want))
    if pts.shape[1] <= LOOP_MAX:
        loop = pm.brute_force(pts, **kw)
        assert pm.same(loop, want) is None, ("loop", pm.same(loop, want))
    return want


CASES = pm.edge_cases()
BY = {c[0]: c for c in CASES}


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_model_loop_and_host_function_agree(name):
    _, pts, kw = BY[name]
    r = _three(pts, **kw)
    n = pts.shape[1]
    fin = np.isfinite(pts).all(0)
    t = np.float64(np.float32(kw["distance_threshold"]))
    # what the rule promises whatever the cloud
    assert r["n_in"] == n and r["n_dropped"] == int((~fin).sum()) and (r["labels"][~fin] == -1).all()
    assert r["n_planes"] <= kw["max_planes"] and r["labels"].max(initial=-1) == r["n_planes"] - 1
    assert r["n_unassigned"] == int(((r["labels"] < 0) & fin).sum())
    left = int(fin.sum())
    for k in range(r["n_planes"]):
        nrm, d, centre, curv = r["model"][k, :3], r["model"][k, 3], r["model"][k, 4:7], r["model"][k, 7]
        h, i0, i1, i2, ransac, final = r["info"][k]
        assert abs(np.linalg.norm(nrm) - 1.0) < 1e-15 and nrm[np.argmax(np.abs(nrm))] > 0
        assert d == -((nrm[0] * centre[0] + nrm[1] * centre[1]) + nrm[2] * centre[2]) and 0.0 <= curv < 1.0 / 3.0 + 1e-15
        assert 0 <= h < kw["n_hypotheses"] and len({i0, i1, i2}) == 3 and 3 <= ransac <= left
        assert final == int((r["labels"] == k).sum()) >= kw["min_inliers"]
        assert (r["labels"][[i0, i1, i2]] >= k).all() or (r["labels"][[i0, i1, i2]] == -1).any()  # samples were open in round k
        on = r["labels"] == k
        assert (np.abs(nrm @ (pts[:, on].astype(np.float64) - centre[:, None])) <= t * (1 + 1e-12)).all()
        left -= final
    assert left == r["n_unassigned"]
    keep = r["out_index"] >= 0
    assert np.array_equal(r["out_index"][keep], np.arange(r["n_out"])) and r["points"].tobytes() == pts[:, keep].tobytes()


def test_constructed_clouds():
    def seg(name, **over):
        _, pts, kw = BY[name]
        return pm.segment(pts, **dict(kw, **over)), pts

    for name in ("empty", "one", "two", "collinear", "identical", "all non-finite", "three, min_inliers 4",
                 "three, 16 draws without three distinct values"):
        r, pts = seg(name)
        assert r["n_planes"] == 0 and r["model"].shape == (0, 8) and (r["labels"] == -1).all(), name
        assert r["n_unassigned"] == r["n_out"] == int(np.isfinite(pts).all(0).sum()), name
    assert pm.sample(pm.NO_SAMPLE_SEED, 0, 3) is None and pm.sample(pm.NO_SAMPLE_SEED, 1, 3) is not None
    # three points: one plane through them, refitted on three points
    r, pts = seg("three, min_inliers 3")
    assert r["n_planes"] == 1 and r["info"][0].tolist()[4:] == [3, 3] and r["n_unassigned"] == 0
    assert r["model"][0].tolist()[:4] == [0.0, 0.0, 1.0, -0.5] and r["model"][0, 7] == 0.0  # the plane z = 0.5
    r, _ = seg("three, the second hypothesis is the first valid one")
    assert r["n_planes"] == 1 and r["info"][0, 0] == 1
    # the <= edge of the count: z = t and z = -t are inliers of a hypothesis in the lattice z = 0, nextafter(t) is not
    r, pts = seg("the <= edge")
    assert pts[2, -3:].tolist() == [0.25, float(np.nextafter(np.float32(0.25), np.float32(1))), -0.25]
    assert r["info"][0, 4] == 122 and (pts[2, r["info"][0, 1:4]] == 0).all()
    # two parallel lattices of equal size: several hypotheses count 64, the lowest h wins; the planes are exact
    counts = []
    r, pts = seg("parallel lattices", counts_out=counts)
    tied = np.flatnonzero(counts[0] == counts[0].max())
    assert counts[0].max() == 64 and tied.size > 1 and r["info"][0, 0] == tied[0]
    assert r["n_planes"] == 2 and r["info"][:, 4:].tolist() == [[64, 64], [64, 64]] and r["n_unassigned"] == 0
    assert np.array_equal(r["model"][:, :3], [[0, 0, 1], [0, 0, 1]]) and sorted(r["model"][:, 3].tolist()) == [-2.0, 0.0]
    for k in range(2):
        assert len(set(pts[2, r["labels"] == k].tolist())) == 1
    r, pts = seg("crossing lattices")
    assert r["n_planes"] == 2 and r["n_unassigned"] == 0
    # scale and offset: the same samples win and the same points are taken
    a, b, c, d = (seg(k)[0] for k in ("scaled 1e-3", "scaled 1e3", "world offset", "non-finite"))
    assert np.array_equal(a["info"], b["info"]) and np.array_equal(a["labels"], b["labels"]) and np.array_equal(a["info"], c["info"])
    assert d["n_dropped"] == 4 and d["n_planes"] == 1
    # rounds: max_planes cuts the third plane off, min_inliers above its final count discards its round
    full, cut, disc = (seg(k)[0] for k in ("three planes", "max_planes reached", "round discarded"))
    assert (full["n_planes"], cut["n_planes"], disc["n_planes"]) == (3, 2, 2)
    assert disc["n_unassigned"] >= 150 > full["info"][2, 5] and pm.same(cut, dict(disc, n_unassigned=cut["n_unassigned"])) is None
    assert np.array_equal(full["info"][:2], cut["info"]) and np.array_equal(full["model"][:2], cut["model"])
    # the selections
    keep_all, keep_1, keep_3 = (seg(k)[0] for k in ("planes kept", "plane 1 kept", "plane 3 kept: there is none"))
    assert np.array_equal(keep_all["keep"], full["labels"] >= 0) and np.array_equal(keep_1["keep"], full["labels"] == 1)
    assert keep_3["n_out"] == 0 and np.array_equal(full["keep"], (full["labels"] < 0))


def test_determinism_and_the_seed():
    _, pts, kw = BY["three planes"]
    a, b = planes.segment_host(pts, **kw), planes.segment_host(pts, **kw)
    assert pm.same(a, b) is None
    # another seed, another winner -- and on the clean lattices the same final mask
    _, lat, lkw = BY["parallel lattices"]
    masks = set()
    winners = set()
    for seed in range(6):
        r = planes.segment_host(lat, **dict(lkw, seed=seed))
        assert r["n_planes"] == 2
        winners.add(tuple(r["info"][0, :4].tolist()))
        masks.add((r["labels"] >= 0).tobytes() + np.sort(r["model"][:, 3]).tobytes())
    assert len(winners) > 1 and len(masks) == 1


def test_refusals_of_the_host_functions():
    lib = binding.load()
    P = binding.PlaneParams
    pts = np.zeros((3, 4), np.float32)
    good = P(0, 0.01, 16, 2, 3, -1, 0)
    none = [None] * 8

    def call(p, flags=0, n=4, points=pts):
        k = C.c_int32(5)
        rc = lib.icpk_segment_planes_host(binding._fp(points) if points is not None else None, n, C.byref(p) if p else None, flags,
                                          C.byref(k), *none[:7])
        assert rc == binding.OK or k.value == 0
        return rc

    assert call(good) == binding.OK and call(good, binding.PLANE_KEEP_INLIERS | binding.PLANE_LABELS_ONLY) == binding.OK
    bad = [P(0, 0.0, 16, 2, 3, -1, 0), P(0, -0.01, 16, 2, 3, -1, 0), P(0, float("nan"), 16, 2, 3, -1, 0),
           P(0, float("inf"), 16, 2, 3, -1, 0), P(0, 0.01, 0, 2, 3, -1, 0), P(0, 0.01, binding.PLANE_MAX_HYPOTHESES + 1, 2, 3, -1, 0),
           P(0, 0.01, 16, 0, 3, -1, 0), P(0, 0.01, 16, binding.PLANE_MAX_PLANES + 1, 3, -1, 0), P(0, 0.01, 16, 2, 2, -1, 0),
           P(0, 0.01, 16, 2, 3, -2, 0), P(0, 0.01, 16, 2, 3, binding.PLANE_MAX_PLANES, 0)]
    for p in bad:
        assert call(p, binding.PLANE_KEEP_INLIERS) == binding.E_ARG, bytes(p)
    assert call(P(0, 0.01, 16, 2, 3, 0, 0), 0) == binding.E_ARG  # select_plane without KEEP_INLIERS
    assert call(P(0, 0.01, 16, 2, 3, 0, 0), binding.PLANE_KEEP_INLIERS) == binding.OK
    assert call(good, 4) == binding.E_ARG and call(good, -1) == binding.E_ARG
    assert call(None) == binding.E_ARG and call(good, n=-1) == binding.E_ARG and call(good, points=None) == binding.E_ARG
    assert call(good, n=0, points=None) == binding.OK
    assert call(P(0, 0.01, binding.PLANE_MAX_HYPOTHESES, binding.PLANE_MAX_PLANES, 3, binding.PLANE_MAX_PLANES - 1, 0),
                binding.PLANE_KEEP_INLIERS) == binding.OK
    d = planes.default_params()
    assert (d.seed, d.distance_threshold, d.n_hypotheses, d.max_planes, d.min_inliers, d.select_plane, d.reserved) == \
        (0, np.float32(0.01), 256, 4, 1000, -1, 0)
    dp = C.POINTER(C.c_double)
    nine, three, eight = np.zeros(9), np.zeros(3), np.zeros(8)
    assert lib.icpk_plane_fit_host(nine.ctypes.data_as(dp), 0, binding._fp(pts), three.ctypes.data_as(dp), eight.ctypes.data_as(dp)) == binding.E_ARG
    assert lib.icpk_plane_fit_host(None, 3, binding._fp(pts), three.ctypes.data_as(dp), eight.ctypes.data_as(dp)) == binding.E_ARG


def _random_inliers(rng):
    """a plane of random orientation, extent (1e-2 .. 1e2), noise and place, 3 .. 3000 points"""
    k = int(rng.integers(3, 3000))
    nrm = rng.normal(size=3)
    nrm /= np.linalg.norm(nrm)
    e1 = np.cross(nrm, rng.normal(size=3))
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    scale = 10.0 ** rng.uniform(-2, 2)
    sigma = scale * 10.0 ** rng.uniform(-4, -1.5)
    uv = rng.uniform(-1, 1, (2, k)) * scale * rng.uniform(0.2, 1.0, (2, 1))
    p = e1[:, None] * uv[0] + e2[:, None] * uv[1] + nrm[:, None] * rng.normal(0, sigma, k) + rng.uniform(-5, 5, (3, 1)) * scale
    return p.astype(np.float32)


def _sums(p, a):
    e = p.astype(np.float64) - a.astype(np.float64)[:, None]
    return np.stack([e[0], e[1], e[2], e[0] * e[0], e[0] * e[1], e[0] * e[2], e[1] * e[1], e[1] * e[2], e[2] * e[2]], axis=1).sum(0)


# Measured here over the 1 000 sets below (seed 34): the worst angle between the refit's normal and numpy.linalg.eigh's
# eigenvector of the same covariance is 2.7e-15 rad, and the centre equals a + S / k computed by numpy exactly (the same
# three operations).  Asserted: ten times the worst value seen.
FIT_ANGLE_TOL = 10 * 2.7e-15
FIT_CENTRE_TOL = 10 * 0.0


def test_refit_against_eigh():
    rng = np.random.default_rng(34)
    worst_angle = worst_centre = 0.0
    for _ in range(1000):
        p = _random_inliers(rng)
        k, a = p.shape[1], p[:, 0]
        S = _sums(p, a)
        got = planes.fit_host(S, k, a, [0.0, 0.0, 1.0])
        want, fitted = pm.fit(S, k, a, [0.0, 0.0, 1.0])
        assert fitted and got.tobytes() == want.tobytes()
        cov = np.array([[S[3] - S[0] * S[0] / k, S[4] - S[0] * S[1] / k, S[5] - S[0] * S[2] / k],
                        [0.0, S[6] - S[1] * S[1] / k, S[7] - S[1] * S[2] / k], [0.0, 0.0, S[8] - S[2] * S[2] / k]])
        w, v = np.linalg.eigh(cov + np.triu(cov, 1).T)
        n = v[:, 0]
        angle = float(np.arctan2(np.linalg.norm(np.cross(n, got[:3])), abs(float(n @ got[:3]))))
        centre = float(np.abs(a.astype(np.float64) + S[:3] / k - got[4:7]).max())
        worst_angle, worst_centre = max(worst_angle, angle), max(worst_centre, centre)
        assert abs(got[7] - w[0] / w.sum()) < 1e-12
    print(f"refit against eigh over 1000 sets: worst angle {worst_angle:.3e} rad, worst centre difference {worst_centre:.3e}")
    assert worst_angle <= FIT_ANGLE_TOL and worst_centre <= FIT_CENTRE_TOL


def test_refit_fallbacks():
    a = np.float32([1.0, 2.0, 3.0])
    N = np.array([0.0, 3.0, -4.0])  # (the sign convention turns it round)
    hyp = np.array([0.0, -0.6, 0.8, -(-0.6 * 2.0 + 0.8 * 3.0), 1.0, 2.0, 3.0, 0.0])
    # inliers on a line; all inliers identical; sums that are not finite: the hypothesis' plane, oriented
    t = np.arange(50, dtype=np.float64) * 0.125
    line = (a.astype(np.float64)[:, None] + np.stack([t, 0 * t, 0 * t])).astype(np.float32)
    for S, k in ((_sums(line, a), 50), (np.zeros(9), 7), (np.full(9, np.inf), 5), (np.full(9, np.nan), 5)):
        got = planes.fit_host(S, k, a, N)
        want, fitted = pm.fit(S, k, a, N)
        assert not fitted and got.tobytes() == want.tobytes()
        assert np.array_equal(got[:3], hyp[:3]) and got[3] == hyp[3] and np.array_equal(got[4:], hyp[4:])
    # nearly a line, but not below 2^-20: a fit
    wide = line.copy()
    wide[1, ::2] += np.float32(0.01)
    wide[2, ::3] += np.float32(0.001)
    got = planes.fit_host(_sums(wide, a), 50, a, N)
    assert pm.fit(_sums(wide, a), 50, a, N)[1] and got.tobytes() == pm.fit(_sums(wide, a), 50, a, N)[0].tobytes() and got[7] > 0


# ---- what it finds in config 2's target (model = host function; the device test holds the library to the same record) --
@pytest.fixture(scope="module")
def target():
    return synth.kinect_pair()["target"]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_usefulness_on_config2(target, seed):
    kw = dict(distance_threshold=0.01, n_hypotheses=256, max_planes=4, min_inliers=5000, seed=seed)
    r = _three(target, **kw)
    pm.check_usefulness(r, target, seed)
    assert r["info"][:, 5].tolist() == [74885, 6468] and r["n_unassigned"] == 10817


def test_min_inliers_is_what_keeps_slices_of_the_sphere_out(target):
    """the reason for the parameter, not a quality bar: at min_inliers = 500 more than two planes come out, and the extra
    ones consist of sphere points only"""
    r = _three(target, distance_threshold=0.01, n_hypotheses=256, max_planes=4, min_inliers=500, seed=0)
    assert r["n_planes"] > 2
    near_sphere = pm.sphere_distance(target) <= 0.02
    print("planes at min_inliers 500:", r["info"][:, 5].tolist())
    assert near_sphere[r["labels"] >= 2].all() and not near_sphere[(r["labels"] == 0) | (r["labels"] == 1)].any()
