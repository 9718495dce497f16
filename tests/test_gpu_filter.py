"""Outlier removal on the device (icpk_remove_outliers, K13) against the numpy model of the rule
(tests/filter_model.py): every per-point value, the sums' summary, the keep mask and the filtered cloud bit for bit --
no tolerance anywhere --, then the state a call leaves behind and alignments that run on filtered clouds."""
import numpy as np
import pytest

import filter_model as fm
import normals_model as nm
from icp_slam_prototype_amd import binding, build, synth

pytestmark = pytest.mark.gpu

CAM = (5.0, 5.0, 5.0)


@pytest.fixture(scope="module")
def ctx():
    build.build()
    c = binding.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def kinect():
    return synth.kinect_pair()


_clouds = {}


def cloud(name):
    if name not in _clouds:
        if name == "config2":
            _clouds[name] = synth.kinect_pair()["target"]
        elif name == "dense307k":
            _clouds[name] = synth.kinect_pair(valid=1.0, seed=6)["target"]
        elif name == "config3":
            fx, cx = float(synth.K2_FX), float(synth.K2_CX)
            _clouds[name] = synth.kinect_pair(rows=424, cols=512, valid=1.0, seed=3, noise_sigma=0.0005, fx=fx, cx=cx)["target"]
        elif name == "config5_200k":
            _clouds[name] = np.ascontiguousarray(synth.dense_pair()["target"][:, :200000])
    return _clouds[name]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def run(ctx, pts, which=1, normals=None, **kw):
    """the call on a fresh upload of pts, and everything it leaves behind"""
    if which == 1:
        ctx.set_target(pts)
        if normals is not None:
            ctx.set_target_normals(normals)
    else:
        ctx.set_source(pts)
    n_out, n_drop = ctx.remove_outliers(which, **kw)
    st = ctx.outlier_stats()
    st["n_dropped"] = n_drop
    assert st["n_out"] == n_out and st["n_in"] == pts.shape[1]
    st["points"] = ctx.get_target() if which == 1 else ctx.get_source()
    if normals is not None:
        st["normals"] = ctx.get_target_normals()
    return st


def check(got, want, name):
    """bit for bit: float and double compared as integers"""
    assert np.array_equal(bits(got["value"]), bits(want["value"])), f"{name}: value differs at " \
        f"{np.flatnonzero(bits(got['value']) != bits(want['value']))[:5]}"
    if want["kth"] is not None:
        assert np.array_equal(bits(got["kth"]), bits(want["kth"])), f"{name}: kth"
    assert np.array_equal(bits(got["summary"]), bits(want["summary"])), (name, got["summary"], want["summary"])
    assert np.array_equal(got["out_index"], want["out_index"]), f"{name}: out_index"
    assert (got["n_out"], got["n_dropped"]) == (want["n_out"], want["n_dropped"]), name
    assert got["points"].shape == want["points"].shape and got["points"].tobytes() == want["points"].tobytes(), name
    if "normals" in want:
        assert got["normals"].tobytes() == want["normals"].tobytes(), f"{name}: normals"


@pytest.mark.parametrize("k", [1, 8, 16, 50, 64])
@pytest.mark.parametrize("name", ["config2", "dense307k", "config3", "config5_200k"])
def test_statistical_parity(ctx, name, k):
    pts = cloud(name)
    which = 0 if (name, k) in (("config2", 8), ("config3", 16)) else 1  # (the source's own index, too)
    got = run(ctx, pts, which, kind=binding.FILTER_STATISTICAL, k=k, std_ratio=2.0)
    want = fm.remove_outliers(pts, fm.STATISTICAL, k=k, std_ratio=2.0)
    print(f"{name} k {k}: n_out {got['n_out']} of {pts.shape[1]}, summary {got['summary']}")
    check(got, want, f"{name} k={k}")


def test_statistical_carries_normals(ctx, kinect):
    tgt = kinect["target"][:, :40000]
    nrm = np.random.default_rng(3).normal(0, 1, tgt.shape).astype(np.float32)
    got = run(ctx, tgt, 1, normals=nrm, kind=binding.FILTER_STATISTICAL, k=16, std_ratio=1.0)
    want = fm.remove_outliers(tgt, fm.STATISTICAL, k=16, std_ratio=1.0, normals=nrm)
    assert 0 < want["n_out"] < tgt.shape[1]
    check(got, want, "normals")


@pytest.mark.parametrize("name,r,min_nb", [("config2", 0.05, 5), ("config2", 0.02, 8), ("config3", 0.03, 20)])
def test_radius_equals_k12_and_model(ctx, name, r, min_nb):
    """m_i equals K12's count[] on the same target and radius -- an independent implementation -- and the model's."""
    pts = cloud(name)
    ctx.set_target(pts)
    ctx.estimate_target_normals(r, 5, CAM)
    k12 = ctx.get_normal_stats()["count"]
    nrm = ctx.get_target_normals()
    got = run(ctx, pts, 1, normals=nrm, kind=binding.FILTER_RADIUS, radius=r, min_neighbors=min_nb)
    assert got["kth"] is None
    assert np.array_equal(got["value"], k12.astype(np.float64))
    want = fm.remove_outliers(pts, fm.RADIUS, radius=r, min_neighbors=min_nb, normals=nrm)
    check(got, want, f"radius {name}")
    src = run(ctx, pts, 0, kind=binding.FILTER_RADIUS, radius=r, min_neighbors=min_nb)
    del want["normals"]
    check(src, want, f"radius {name} as source")


def test_radius_lattice_wall_ties(ctx):
    """r equal to a lattice distance: the float `<=` decides, as in K12"""
    w = synth.lattice_wall()["target"]
    d = nm.pair_dist(w[:, :1], w[:, 1:2])[0]
    for r in (float(d), float(np.nextafter(d, np.float32(0)))):
        got = run(ctx, w, 1, kind=binding.FILTER_RADIUS, radius=r, min_neighbors=3)
        check(got, fm.remove_outliers(w, fm.RADIUS, radius=r, min_neighbors=3), f"lattice r={r}")
        ctx.set_target(w)
        ctx.estimate_target_normals(r, 3, CAM)
        assert np.array_equal(got["value"], ctx.get_normal_stats()["count"].astype(np.float64))
    got = run(ctx, w, 1, kind=binding.FILTER_STATISTICAL, k=8, std_ratio=0.5)
    check(got, fm.remove_outliers(w, fm.STATISTICAL, k=8, std_ratio=0.5), "lattice knn (ties at the k-th place)")


def edge_clouds():
    rng = np.random.default_rng(17)
    base = rng.uniform(-0.5, 0.5, (3, 3000)).astype(np.float32)
    dup = base.copy()
    dup[:, 1000:1500] = dup[:, :500]
    dup[:, 1500:1600] = dup[:, 0:1]
    nonfin = base.copy()
    nonfin[1, 1500] = np.nan
    nonfin[0, 1501] = np.inf
    nonfin[2, 1502] = -np.inf
    far = base.copy()
    far[:, 777] = np.float32([40.0, 35.0, -30.0])  # the search radius of this one grows to the whole grid
    return [("duplicates", dup), ("identical", np.tile(np.float32([[1.0], [2.0], [3.0]]), (1, 500))),
            ("one", base[:, :1]), ("two", base[:, :2]), ("k>=N", base[:, :12]), ("non-finite", nonfin),
            ("scaled 1e-3", base * np.float32(1e-3)), ("scaled 1e3", base * np.float32(1e3)),
            ("one cell", base[:, :5]), ("isolated", far), ("empty", np.zeros((3, 0), np.float32))]


@pytest.mark.parametrize("which", [0, 1])
def test_edges(ctx, which):
    for name, pts in edge_clouds():
        pts = np.ascontiguousarray(pts)
        for k in (1, 16, 64):
            got = run(ctx, pts, which, kind=binding.FILTER_STATISTICAL, k=k, std_ratio=1.0)
            check(got, fm.remove_outliers(pts, fm.STATISTICAL, k=k, std_ratio=1.0), f"{name} k={k} which={which}")
        scale = 1e-3 if name == "scaled 1e-3" else 1e3 if name == "scaled 1e3" else 1.0
        got = run(ctx, pts, which, kind=binding.FILTER_RADIUS, radius=0.08 * scale, min_neighbors=4)
        check(got, fm.remove_outliers(pts, fm.RADIUS, radius=0.08 * scale, min_neighbors=4), f"{name} radius which={which}")
    # every point removed -> an empty cloud
    pts = edge_clouds()[0][1]
    got = run(ctx, pts, which, kind=binding.FILTER_RADIUS, radius=1e-6, min_neighbors=1000)
    assert got["n_out"] == 0 and got["points"].shape == (3, 0) and (got["out_index"] == -1).all()


def test_refusals(kinect):
    with binding.Context(0) as c:
        F = binding.OutlierFilter
        lib, h = c._lib, c._h
        import ctypes as C
        ok = F(0, 16, 2.0, 0.05, 5)
        assert lib.icpk_remove_outliers(h, 1, C.byref(ok), 0, None, None) == binding.E_NOT_SET
        assert lib.icpk_remove_outliers(h, 0, C.byref(ok), 0, None, None) == binding.E_NOT_SET
        assert lib.icpk_get_outlier_stats(h, None, None, None, None, None, None) == binding.E_NOT_SET
        tgt = kinect["target"][:, :5000]
        c.set_target(tgt)
        bad = [(2, ok, 0), (-1, ok, 0), (1, ok, 2), (1, F(2, 16, 2.0, 0.05, 5), 0), (1, F(0, 0, 2.0, 0.05, 5), 0),
               (1, F(0, 65, 2.0, 0.05, 5), 0), (1, F(0, 16, -1.0, 0.05, 5), 0), (1, F(0, 16, float("nan"), 0.05, 5), 0),
               (1, F(0, 16, float("inf"), 0.05, 5), 0), (1, F(1, 16, 2.0, 0.0, 5), 0), (1, F(1, 16, 2.0, float("inf"), 5), 0),
               (1, F(1, 16, 2.0, float("nan"), 5), 0), (1, F(1, 16, 2.0, 0.05, 0), 0)]
        for which, f, flags in bad:
            assert lib.icpk_remove_outliers(h, which, C.byref(f), flags, None, None) == binding.E_ARG, (which, flags)
        assert lib.icpk_remove_outliers(h, 1, None, 0, None, None) == binding.E_ARG
        assert lib.icpk_get_outlier_stats(h, None, None, None, None, None, None) == binding.E_NOT_SET
        assert c.get_target().tobytes() == tgt.tobytes()
        # only the fields of the kind are read
        assert lib.icpk_remove_outliers(h, 1, C.byref(F(0, 16, 2.0, -1.0, 0)), 0, None, None) == binding.OK


def _trace_bytes(c):
    return [(t["R"].tobytes(), t["t"].tobytes(), t["n_pairs"], t["mse"].tobytes()) for t in c.get_trace()]


def _align_bytes(c, **kw):
    T, st, rc = c.align(**kw)
    return rc, T.tobytes(), st.iterations, st.final_pairs, np.float32(st.final_mse).tobytes(), _trace_bytes(c)


def test_state(kinect):
    tgt, src = kinect["target"], kinect["source"]
    kw = dict(max_iterations=6, fixed_iterations=1)
    p2l = dict(solve=binding.SOLVE_POINT_TO_PLANE, max_iterations=6, fixed_iterations=1, max_nn_dist=0.3)
    with binding.Context(0) as fresh:
        fresh.set_target(tgt)
        fresh.set_source(src)
        plain = _align_bytes(fresh, **kw)
        fresh.estimate_target_normals(0.05, 5, CAM)
        nrm = fresh.get_target_normals()
        fresh.set_source(src)
        plain_p2l = _align_bytes(fresh, **p2l)
    # STATS_ONLY changes nothing: clouds, normals, then an alignment -- on either cloud, before and after an index exists
    with binding.Context(0) as c:
        c.set_target(tgt)
        c.set_source(src)
        for which in (1, 0):
            n_out, _ = c.remove_outliers(which, k=16, std_ratio=1.0, stats_only=True)
            assert 0 < n_out < (src, tgt)[which].shape[1]
        assert c.get_target().tobytes() == tgt.tobytes() and c.get_source().tobytes() == src.tobytes()
        assert _align_bytes(c, **kw) == plain
        c.estimate_target_normals(0.05, 5, CAM)
        c.set_source(src)
        c.remove_outliers(1, kind=binding.FILTER_RADIUS, radius=0.05, min_neighbors=5, stats_only=True)
        c.remove_outliers(0, k=8, stats_only=True)
        assert c.get_target_normals().tobytes() == nrm.tobytes() and c.get_normal_stats()["n"] == tgt.shape[1]
        assert _align_bytes(c, **p2l) == plain_p2l
    # which = 0 leaves the target's index alone: the bits of a fresh context on the same two clouds
    want_s = fm.remove_outliers(src, fm.STATISTICAL, k=16, std_ratio=1.0)
    want_t = fm.remove_outliers(tgt, fm.STATISTICAL, k=16, std_ratio=1.0, normals=nrm)
    with binding.Context(0) as c, binding.Context(0) as ref:
        c.set_target(tgt)
        c.set_source(src)
        c.align(**kw)  # (the target's index exists and the source has moved)
        c.set_source(src)
        assert c.remove_outliers(0, k=16, std_ratio=1.0) == (want_s["n_out"], 0)
        assert c.get_source().tobytes() == want_s["points"].tobytes()
        ref.set_target(tgt)
        ref.set_source(want_s["points"])
        assert _align_bytes(c, **kw) == _align_bytes(ref, **kw)
        # a replacing call on the target: K12's record is gone, the normals are carried, the next alignment equals one
        # on set_target(cloud[keep])
        c.estimate_target_normals(0.05, 5, CAM)
        assert c.remove_outliers(1, k=16, std_ratio=1.0) == (want_t["n_out"], 0)
        with pytest.raises(binding.IcpkError) as e:
            c.get_normal_stats()
        assert e.value.code == binding.E_NOT_SET
        assert c.get_target().tobytes() == want_t["points"].tobytes()
        assert c.get_target_normals().tobytes() == want_t["normals"].tobytes()
        ref.set_target(want_t["points"])
        ref.set_target_normals(want_t["normals"])
        c.set_source(want_s["points"])
        ref.set_source(want_s["points"])
        assert _align_bytes(c, **p2l) == _align_bytes(ref, **p2l)
        # the moved working source is what which = 0 filters
        moved = c.get_source()
        assert not np.array_equal(moved, want_s["points"])
        c.remove_outliers(0, kind=binding.FILTER_RADIUS, radius=0.05, min_neighbors=6)
        assert c.get_source().tobytes() == fm.remove_outliers(moved, fm.RADIUS, radius=0.05, min_neighbors=6)["points"].tobytes()


def test_same_bits_on_two_runs(ctx, kinect):
    tgt = kinect["target"]
    a = run(ctx, tgt, 1, k=16, std_ratio=2.0)
    b = run(ctx, tgt, 1, k=16, std_ratio=2.0)
    for key in ("value", "kth", "summary", "out_index", "points"):
        assert a[key].tobytes() == b[key].tobytes(), key
    # the per-point values do not depend on the order of the cloud (S1 / S2, hence T, may)
    perm = np.random.default_rng(4).permutation(tgt.shape[1])
    m = run(ctx, np.ascontiguousarray(tgt[:, perm]), 1, k=16, std_ratio=2.0, stats_only=True)
    assert m["value"].tobytes() == a["value"][perm].tobytes() and m["kth"].tobytes() == a["kth"][perm].tobytes()


def test_usefulness_on_the_device(ctx, kinect):
    """The mask of tests/test_filter_host.py's usefulness test, once on the GPU: config 2's target plus 2 % strays,
    STATISTICAL k = 16, alpha = 2 removes >= 90 % of the strays and <= 5 % of the genuine points (the model: 93.33 % /
    0.00 %), RADIUS r = 0.05, min_neighbors = 5 likewise (96.91 % / 0.01 %)."""
    pts, stray = fm.with_strays(kinect["target"])
    for kw in (dict(kind=binding.FILTER_STATISTICAL, k=16, std_ratio=2.0),
               dict(kind=binding.FILTER_RADIUS, radius=0.05, min_neighbors=5)):
        got = run(ctx, pts, 1, **kw)
        keep = got["out_index"] >= 0
        s, g = 1.0 - keep[stray].mean(), 1.0 - keep[~stray].mean()
        print(f"{kw}: strays removed {100 * s:.2f} %, genuine removed {100 * g:.2f} %")
        assert s >= 0.90 and g <= 0.05
        assert np.array_equal(keep, fm.remove_outliers(pts, **kw)["keep"])


def test_config3_with_strays_end_to_end(ctx):
    """Config 3 from plain clouds with 2 % strays in both clouds, 15 fixed point-to-plane iterations on K12 normals
    (r = 0.03, min_neighbors = 5), with and without STATISTICAL (k = 16, alpha = 2) on both clouds.  Measured on an
    MI355X: unfiltered |R - R_true| 4.115e-4, |t - t_true| 2.327e-3, 216 063 pairs; filtered 4.719e-4, 2.519e-3, 217 227
    pairs; 217 117 target points with a normal in BOTH runs.  The filtered run is not the better one, so no ordering is
    asserted: a stray has fewer than 5 neighbours within 3 cm, gets no normal from K12 and never pairs under
    point-to-plane, filtered or not.  Asserted: both runs return ICPK_OK and the filtered clouds equal
    the model's."""
    fx, cx = float(synth.K2_FX), float(synth.K2_CX)
    p = synth.kinect_pair(rows=424, cols=512, valid=1.0, seed=3, noise_sigma=0.0005, fx=fx, cx=cx)
    o = np.full(3, 5.0)
    t_full = o - p["R_true"] @ o + p["t_true"]
    tgt, _ = fm.with_strays(p["target"], seed=7)
    src, _ = fm.with_strays(p["source"], seed=8)
    kw = dict(solve=binding.SOLVE_POINT_TO_PLANE, max_iterations=15, fixed_iterations=1, max_nn_dist=0.3)
    res = {}
    for filtered in (False, True):
        ctx.set_target(tgt)
        ctx.set_source(src)
        if filtered:
            nt, _ = ctx.remove_outliers(1, k=16, std_ratio=2.0)
            ns, _ = ctx.remove_outliers(0, k=16, std_ratio=2.0)
            assert ctx.get_target().tobytes() == fm.remove_outliers(tgt, k=16, std_ratio=2.0)["points"].tobytes()
            assert ctx.get_source().tobytes() == fm.remove_outliers(src, k=16, std_ratio=2.0)["points"].tobytes()
        ctx.estimate_target_normals(0.03, 5, CAM)
        valid = ctx.get_normal_stats()["n_valid"]
        T, st, rc = ctx.align(**kw)
        assert rc == binding.OK
        T = T.astype(np.float64)
        res[filtered] = (np.linalg.norm(T[:3, :3] - p["R_true"]), np.linalg.norm(T[:3, 3] - t_full), st.final_pairs, valid,
                         ctx.target_size, ctx.source_size)
        print(f"config 3 + 2 % strays, filtered={filtered}: |R - R_true| {res[filtered][0]:.3e} |t - t_true| "
              f"{res[filtered][1]:.3e} pairs {st.final_pairs} normals {valid} target {ctx.target_size} source {ctx.source_size}")
