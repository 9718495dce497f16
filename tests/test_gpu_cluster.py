"""DBSCAN clustering on the device (icpk_cluster_dbscan, K33) against the numpy model of THE CLUSTER RULE
(tests/cluster_model.py): every array of the record and the selected cloud bit for bit -- no tolerance anywhere --, the
counts against K12's and K13's, the state a call leaves behind, reused contexts and threads, what clustering removes that
the radius filter keeps, and alignments that run on clustered clouds."""
import ctypes as C
import threading
import traceback

import numpy as np
import pytest

import cluster_model as cm
import history_cases as hc
from icp_slam_prototype_amd import binding, build, cluster, synth

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


_models = {}


def model(key, pts, eps, mp, **sel):
    """the model's record of a named cloud, computed once and left unchanged"""
    k = (key, eps, mp, tuple(sorted(sel.items())))
    if k not in _models:
        _models[k] = cm.dbscan(pts, eps, mp, **sel)
    return _models[k]


def run(ctx, pts, eps, mp, which=1, normals=None, upload=True, **kw):
    """the call on a fresh upload of pts, and everything it leaves behind"""
    if upload:
        if which == 1:
            ctx.set_target(pts)
            if normals is not None:
                ctx.set_target_normals(normals)
        else:
            ctx.set_source(pts)
    nc, noise, n_out = cluster.dbscan(ctx, which, eps, mp, **kw)
    rec = cluster.clusters(ctx)
    assert (rec["n_clusters"], rec["n_noise"], rec["n_out"]) == (nc, noise, n_out) and rec["n_in"] == pts.shape[1]
    rec["points"] = ctx.get_target() if which == 1 else ctx.get_source()
    if normals is not None:
        rec["normals"] = ctx.get_target_normals()
    return rec


def check(got, want, name):
    """bit for bit: every array compared as bytes"""
    assert cm.same(got, want) is None, (name, cm.same(got, want))
    if "normals" in want:
        assert got["normals"].tobytes() == want["normals"].tobytes(), f"{name}: normals"


def record_bytes(rec):
    return b"".join(np.ascontiguousarray(rec[k]).tobytes() for k in cm.FIELDS)


# (eps, min_points) -> clusters, noise, border points of config 2's target, by the model on the CPU
CONFIG2 = {(0.05, 5): (2, 0, 10), (0.02, 8): (2374, 21189, 32170), (0.03, 1): (15, 0, 0)}


@pytest.mark.parametrize("eps,mp", list(CONFIG2))
def test_parity_on_config2(ctx, kinect, eps, mp):
    tgt = kinect["target"]
    want = model("config2", tgt, eps, mp)
    border = int(((want["core"] == 0) & (want["labels"] >= 0)).sum())
    print(f"config 2 target ({eps}, {mp}): {want['n_clusters']} clusters, {want['n_noise']} noise, {border} border")
    assert (want["n_clusters"], want["n_noise"], border) == CONFIG2[(eps, mp)]
    check(run(ctx, tgt, eps, mp, 1), want, f"target ({eps}, {mp})")
    if (eps, mp) == (0.02, 8):  # the source's own index, on the setting that takes every branch
        check(run(ctx, tgt, eps, mp, 0), want, "as the source")
        nrm = np.random.default_rng(3).normal(0, 1, tgt.shape).astype(np.float32)
        sel = dict(min_size=20, max_size=3000)
        want = model("config2", tgt, eps, mp, **sel)
        assert 0 < want["n_out"] < tgt.shape[1] - want["n_noise"]
        want = dict(want, normals=nrm[:, want["keep"]])
        check(run(ctx, tgt, eps, mp, 1, normals=nrm, **sel), want, "selected by size, normals carried")
    if mp == 1:
        got = cluster.clusters(ctx)
        assert not (got["labels"] < 0).any() and (got["core"] == 1).all()  # no noise among finite points


@pytest.mark.parametrize("which", [0, 1])
def test_edge_clouds(ctx, which):
    for name, pts, eps, mp in cm.edge_cases():
        check(run(ctx, pts, eps, mp, which), cm.dbscan(pts, eps, mp), f"{name} which={which}")
    # every point removed -> an empty cloud; the largest of two equal clusters is the lower label
    name, pts, eps, mp = next(c for c in cm.edge_cases() if c[0] == "random, sparse")
    got = run(ctx, pts, eps, mp, which, min_size=10 ** 6)
    assert got["n_out"] == 0 and got["points"].shape == (3, 0) and (got["out_index"] == -1).all()
    t = np.concatenate([np.arange(5) * 0.01, 1.0 + np.arange(9) * 0.01, 2.0 + np.arange(5) * 0.01, [3.0]])
    line = np.stack([t, 0 * t, 0 * t]).astype(np.float32)
    for sel in (dict(largest_only=True), dict(min_size=0, max_size=5), dict(min_size=5, max_size=5), dict(largest_only=True, max_size=5)):
        check(run(ctx, line, 0.011, 2, which, **sel), cm.dbscan(line, 0.011, 2, **sel), f"line {sel}")
    tie = np.ascontiguousarray(line[:, [0, 1, 2, 3, 4, 14, 15, 16, 17, 18, 19]])
    got = run(ctx, tie, 0.011, 2, which, largest_only=True)
    check(got, cm.dbscan(tie, 0.011, 2, largest_only=True), "tie in size")
    assert got["sizes"].tolist() == [5, 5] and got["n_out"] == 5 and (got["out_index"][:5] >= 0).all()


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_chain_of_20000_is_one_cluster(ctx, order):
    """the deep-tree case: every point is linked to its two neighbours on the line only"""
    pts = cm.chain(20000, 0.01, order)
    got = run(ctx, pts, 0.01, 2, 1, labels_only=True)
    assert got["n_clusters"] == 1 and got["sizes"].tolist() == [20000] and got["first"].tolist() == [0] and got["n_noise"] == 0
    check(got, cm.dbscan(pts, 0.01, 2), order)


def test_4096_identical_points(ctx):
    """the contention case: every pair is an edge"""
    pts = np.tile(np.float32([[0.25], [-1.5], [3.0]]), (1, 4096))
    got = run(ctx, pts, 0.01, 5, 1)
    assert got["n_clusters"] == 1 and (got["count"] == 4096).all() and got["first"].tolist() == [0] and got["n_out"] == 4096
    check(got, cm.dbscan(pts, 0.01, 5), "identical")


@pytest.mark.parametrize("r", [0.05, 0.02])
def test_count_equals_k13_and_k12(ctx, kinect, r):
    tgt = kinect["target"]
    ctx.set_target(tgt)
    ctx.estimate_target_normals(r, 5, CAM)
    k12 = ctx.get_normal_stats()["count"]
    ctx.remove_outliers(1, kind=binding.FILTER_RADIUS, radius=r, min_neighbors=5, stats_only=True)
    k13 = ctx.outlier_stats()["value"]
    cluster.dbscan(ctx, 1, r, 5, labels_only=True)
    count = cluster.clusters(ctx)["count"]
    assert np.array_equal(count, k12) and np.array_equal(count.astype(np.float64), k13)


def test_refusals(kinect):
    with binding.Context(0) as c:
        lib, h = c._lib, c._h
        P = binding.ClusterParams
        ok = P(0.05, 5, 1, 0, 0)
        none = (None, None, None)
        assert lib.icpk_cluster_dbscan(h, 1, C.byref(ok), 0, *none) == binding.E_NOT_SET
        assert lib.icpk_cluster_dbscan(h, 0, C.byref(ok), 0, *none) == binding.E_NOT_SET
        assert lib.icpk_get_clusters(h, *[None] * 9) == binding.E_NOT_SET
        tgt = kinect["target"][:, :5000]
        c.set_target(tgt)
        bad = [(2, ok, 0), (-1, ok, 0), (1, ok, 2), (1, ok, -1), (1, P(0.0, 5, 1, 0, 0), 0), (1, P(-0.05, 5, 1, 0, 0), 0),
               (1, P(float("nan"), 5, 1, 0, 0), 0), (1, P(float("inf"), 5, 1, 0, 0), 0), (1, P(0.05, 0, 1, 0, 0), 0),
               (1, P(0.05, 5, -1, 0, 0), 0), (1, P(0.05, 5, 1, -1, 0), 0), (1, P(0.05, 5, 9, 8, 0), 0), (1, P(0.05, 5, 1, 0, 2), 0)]
        for which, p, flags in bad:
            assert lib.icpk_cluster_dbscan(h, which, C.byref(p), flags, *none) == binding.E_ARG, (which, flags, bytes(p))
        assert lib.icpk_cluster_dbscan(h, 1, None, 0, *none) == binding.E_ARG
        assert lib.icpk_get_clusters(h, *[None] * 9) == binding.E_NOT_SET
        assert c.get_target().tobytes() == tgt.tobytes()
        # an empty cloud is no refusal
        c.set_source(np.zeros((3, 0), np.float32))
        assert cluster.dbscan(c, 0, 0.05, 5) == (0, 0, 0)
        rec = cluster.clusters(c)
        assert rec["n_in"] == 0 and rec["labels"].shape == (0,) and rec["sizes"].shape == (0,)


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
    # labels_only changes nothing: clouds, normals, then an alignment -- on either cloud, before and after an index exists
    with binding.Context(0) as c:
        c.set_target(tgt)
        c.set_source(src)
        for which in (1, 0):
            nc, noise, n_out = cluster.dbscan(c, which, 0.02, 8, min_size=20, labels_only=True)
            assert nc > 100 and 0 < n_out < (src, tgt)[which].shape[1]
        assert c.get_target().tobytes() == tgt.tobytes() and c.get_source().tobytes() == src.tobytes()
        assert _align_bytes(c, **kw) == plain
        c.estimate_target_normals(0.05, 5, CAM)
        c.set_source(src)
        cluster.dbscan(c, 1, 0.05, 5, largest_only=True, labels_only=True)
        cluster.dbscan(c, 0, 0.03, 3, labels_only=True)
        assert c.get_target_normals().tobytes() == nrm.tobytes() and c.get_normal_stats()["n"] == tgt.shape[1]
        assert _align_bytes(c, **p2l) == plain_p2l
    # which = 0 leaves the target's index alone: the bits of a fresh context on the same two clouds
    sel = dict(min_size=20)
    want_s = model("config2 source", src, 0.02, 8, **sel)
    want_t = dict(model("config2", tgt, 0.02, 8, **sel))
    want_t["normals"] = nrm[:, want_t["keep"]]
    with binding.Context(0) as c, binding.Context(0) as ref:
        c.set_target(tgt)
        c.set_source(src)
        c.align(**kw)  # (the target's index exists and the source has moved)
        c.set_source(src)
        assert cluster.dbscan(c, 0, 0.02, 8, **sel)[2] == want_s["n_out"]
        assert c.get_source().tobytes() == want_s["points"].tobytes()
        ref.set_target(tgt)
        ref.set_source(want_s["points"])
        assert _align_bytes(c, **kw) == _align_bytes(ref, **kw)
        # a replacing call on the target: K12's record is gone, the normals are carried, the next alignment equals one
        # on set_target(cloud[keep])
        c.estimate_target_normals(0.05, 5, CAM)
        assert cluster.dbscan(c, 1, 0.02, 8, **sel)[2] == want_t["n_out"]
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
        # the moved working source is what which = 0 clusters
        moved = c.get_source()
        assert not np.array_equal(moved, want_s["points"])
        cluster.dbscan(c, 0, 0.03, 4, largest_only=True)
        assert c.get_source().tobytes() == cm.dbscan(moved, 0.03, 4, largest_only=True)["points"].tobytes()


def _probe(c, kinect, variant=0):
    """the feature's surface as bytes: both clouds, labels only and replacing, the settings of the parity test"""
    tgt, src = kinect["target"], kinect["source"]
    eps, mp, sel = ((0.02, 8, dict(min_size=20)), (0.05, 5, dict(largest_only=True)), (0.03, 1, dict(max_size=50000)))[variant % 3]
    out = record_bytes(run(c, tgt, eps, mp, 1, labels_only=True, **sel))
    out += record_bytes(run(c, src, eps, mp, 0, **sel))
    nrm = np.random.default_rng(variant).normal(0, 1, tgt.shape).astype(np.float32)
    rec = run(c, tgt, eps, mp, 1, normals=nrm, **sel)
    return out + record_bytes(rec) + rec["normals"].tobytes()


@pytest.fixture(scope="module")
def serial(kinect):
    out = []
    for v in range(3):
        with binding.Context(0) as c:
            out.append(_probe(c, kinect, v))
    assert len(set(out)) == 3
    return out


def test_two_runs_give_the_same_bytes(ctx, kinect, serial):
    for v in (0, 0, 1):
        assert _probe(ctx, kinect, v) == serial[v], v


@pytest.mark.parametrize("history", ["Q.filter", "S.voxel", "Q.align_point_to_plane", "Q.fpfh", "shared_aux_index", "early_non_finite",
                                     "early_filter_leaves_nothing"])
def test_a_reused_context_gives_a_fresh_contexts_bytes(kinect, serial, history):
    with binding.Context(0) as c:
        hc.HISTORIES[history](c)
        for v in (2, 0):
            assert _probe(c, kinect, v) == serial[v], (history, v)


def test_eight_threads_with_a_context_each_give_the_serial_bytes(kinect, serial):
    got, errors = [None] * 8, []

    def work(k):
        try:
            with binding.Context(0) as c:
                got[k] = _probe(c, kinect, k % 3)
        except Exception:  # noqa: BLE001 -- reported below, with the thread's traceback
            errors.append(traceback.format_exc())

    threads = [threading.Thread(target=work, args=(k,)) for k in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[0]
    for k in range(8):
        assert got[k] == serial[k % 3], k


def test_usefulness_on_the_device(ctx, kinect):
    """Config 2's target plus 40 clumps of 12 strays (seed 11, sigma 4 mm, tests/cluster_model.with_clumps): RADIUS
    (0.05, 5) removes less than 5 % of the strays, clusters of at least 50 points at (0.05, 5) at least 95 % of them and
    at most 0.1 % of the genuine points.  The model alone: 0 % / 100 % / 0."""
    pts, stray = cm.with_clumps(kinect["target"])
    want = cm.dbscan(pts, 0.05, 5, min_size=50)
    got = run(ctx, pts, 0.05, 5, 1, min_size=50)
    check(got, want, "clumps")
    ctx.set_target(pts)
    ctx.remove_outliers(1, kind=binding.FILTER_RADIUS, radius=0.05, min_neighbors=5, stats_only=True)
    rad = ctx.outlier_stats()["out_index"] >= 0
    keep = got["out_index"] >= 0
    s_rad, s_cl, g_cl = 1.0 - rad[stray].mean(), 1.0 - keep[stray].mean(), 1.0 - keep[~stray].mean()
    print(f"strays removed: RADIUS {100 * s_rad:.2f} %, clusters of >= 50 {100 * s_cl:.2f} %; genuine removed {100 * g_cl:.3f} %")
    assert s_rad < 0.05
    assert s_cl >= 0.95 and g_cl <= 0.001


def test_config2_largest_cluster_end_to_end(ctx, kinect):
    """Config 2, the largest cluster of both clouds at (0.05, 5), then icpk_align (Kabsch, 15 fixed iterations), next to
    the same alignment of the whole clouds.  Asserted: both return ICPK_OK and the clustered clouds equal the model's; the
    errors are printed and no ordering is asserted, as K13's end-to-end test asserts none."""
    tgt, src = kinect["target"], kinect["source"]
    kw = dict(solve=binding.SOLVE_KABSCH, max_iterations=15, fixed_iterations=1)
    for clustered in (False, True):
        ctx.set_target(tgt)
        ctx.set_source(src)
        if clustered:
            cluster.dbscan(ctx, 1, 0.05, 5, largest_only=True)
            cluster.dbscan(ctx, 0, 0.05, 5, largest_only=True)
            assert ctx.get_target().tobytes() == model("config2", tgt, 0.05, 5, largest_only=True)["points"].tobytes()
            assert ctx.get_source().tobytes() == model("config2 source", src, 0.05, 5, largest_only=True)["points"].tobytes()
        T, st, rc = ctx.align(**kw)
        assert rc == binding.OK
        T = T.astype(np.float64)
        print(f"config 2, largest cluster only={clustered}: |R - R_true| {np.linalg.norm(T[:3, :3] - kinect['R_true']):.3e} "
              f"pairs {st.final_pairs} target {ctx.target_size} source {ctx.source_size}")
