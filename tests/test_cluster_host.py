"""DBSCAN clustering (K33) without a GPU: the numpy model of THE CLUSTER RULE (tests/cluster_model.py), a literal double
loop with a breadth-first search, and the library's host-only icpk_cluster_host against one another, bit for bit; what
the rule promises on constructed clouds; the refusals of the host function; and what clustering removes from a cloud with
clumps of strays that the radius filter keeps."""
import ctypes as C

import numpy as np
import pytest

import cluster_model as cm
import filter_model as fm
from icp_slam_prototype_amd import binding, build, cluster, synth

LOOP_MAX = 330  # points up to which the Python double loop runs in a moment


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build()


def _three(pts, eps, mp, **sel):
    """the model's record, held to the host function's and (small clouds) the double loop's"""
    want = cm.dbscan(pts, eps, mp, **sel)
    host = cluster.dbscan_host(pts, eps, mp, **sel)
    assert cm.same(host, want) is None, ("host", cm.same(host, want))
    if pts.shape[1] <= LOOP_MAX:
        loop = cm.brute_force(pts, eps, mp, **sel)
        assert cm.same(loop, want) is None, ("loop", cm.same(loop, want))
    return want


CASES = cm.edge_cases()


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_model_loop_and_host_function_agree(name):
    _, pts, eps, mp = next(c for c in CASES if c[0] == name)
    r = _three(pts, eps, mp)
    n = pts.shape[1]
    fin = np.isfinite(pts).all(0)
    # what the rule promises whatever the cloud
    assert r["n_dropped"] == int((~fin).sum()) and np.array_equal(r["count"] == 0, ~fin)
    assert np.array_equal(r["core"] != 0, r["count"] >= mp)
    assert np.array_equal(r["nearest_core"][r["core"] != 0], np.flatnonzero(r["core"]))
    assert np.array_equal(r["labels"] < 0, r["nearest_core"] < 0) and r["n_noise"] == int((r["labels"] < 0).sum())
    assert np.array_equal(r["sizes"], np.bincount(r["labels"][r["labels"] >= 0], minlength=r["n_clusters"]))
    assert (np.diff(r["first"]) > 0).all() and np.array_equal(r["labels"][r["first"]], np.arange(r["n_clusters"]))
    for c, f in enumerate(r["first"]):  # the representative is the smallest core index of its cluster
        assert f == np.flatnonzero((r["labels"] == c) & (r["core"] != 0))[0]
    assert r["n_in"] == n and r["n_out"] == int((r["labels"] >= 0).sum())  # (min_size 1: every labelled point is kept)
    if mp == 1:
        assert not (r["labels"][fin] < 0).any() and (r["core"][fin] == 1).all()


def test_constructed_clouds():
    by = {c[0]: c for c in CASES}
    r = cm.dbscan(*by["empty"][1:])
    assert (r["n_clusters"], r["n_noise"], r["n_out"]) == (0, 0, 0) and r["labels"].shape == (0,)
    assert cm.dbscan(*by["one, min_points 1"][1:])["labels"].tolist() == [0]
    assert cm.dbscan(*by["one, min_points 2"][1:])["labels"].tolist() == [-1]
    r = cm.dbscan(*by["two at eps, min_points 2"][1:])  # d == eps exactly: the float `<=` makes them neighbours
    assert r["labels"].tolist() == [0, 0] and r["count"].tolist() == [2, 2]
    assert cm.dbscan(*by["two at eps, min_points 3"][1:])["labels"].tolist() == [-1, -1]
    assert cm.dbscan(*by["two below eps apart"][1:])["labels"].tolist() == [-1, -1]
    r = cm.dbscan(*by["identical"][1:])
    assert r["n_clusters"] == 1 and (r["count"] == 300).all() and r["first"].tolist() == [0]
    assert cm.dbscan(*by["identical, min_points above n"][1:])["n_clusters"] == 0
    r = cm.dbscan(*by["non-finite"][1:])
    assert (r["labels"][[700, 701, 702]] == -1).all() and (r["count"][[700, 701, 702]] == 0).all() and r["n_dropped"] == 3
    r = cm.dbscan(*by["all non-finite"][1:])
    assert r["n_clusters"] == 0 and r["n_noise"] == 5 and r["n_dropped"] == 5
    r = cm.dbscan(*by["lattice wall"][1:])  # an inner point has itself and six at exactly eps; a face point five
    assert int(r["count"].max()) == 7 and r["n_clusters"] == 1 and 0 < int((r["core"] == 0).sum()) < r["n_in"]
    for order in ("ascending", "descending", "shuffled"):
        r = cm.dbscan(*by[f"chain 2000 {order}"][1:])
        assert r["n_clusters"] == 1 and r["n_noise"] == 0 and r["sizes"].tolist() == [2000] and r["first"].tolist() == [0]


def test_a_border_point_joins_no_clusters_together():
    pts, k = cm.bridge(False)
    r = _three(pts, 1.0, 8)
    assert r["n_clusters"] == 2 and r["sizes"].tolist() == [27, 28] and r["core"][k] == 0
    assert r["labels"][k] == 1 and r["nearest_core"][k] == 27 + 4  # the centre of the second blob's near face
    assert (r["labels"][:27] == 0).all() and (r["labels"][27:54] == 1).all()
    pts, k = cm.bridge(True)  # the same float distance to one core point of each blob: the lower index
    d = cm.pair_dist(pts[:, [k, k]], pts[:, [13 + 9, 27 + 4]])
    assert d[0] == d[1] == np.float32(0.875)
    r = _three(pts, 1.0, 8)
    assert r["n_clusters"] == 2 and r["sizes"].tolist() == [28, 27] and r["labels"][k] == 0 and r["nearest_core"][k] == 22


def test_core_partition_of_a_permuted_cloud_is_the_permuted_partition():
    rng = np.random.default_rng(23)
    pts = rng.uniform(-0.5, 0.5, (3, 1200)).astype(np.float32)
    eps, mp = 0.07, 5
    a = cm.dbscan(pts, eps, mp)
    assert a["n_clusters"] > 3 and a["n_noise"] > 0 and int(((a["core"] == 0) & (a["labels"] >= 0)).sum()) > 0
    perm = rng.permutation(pts.shape[1])  # new index k holds old point perm[k]
    q = np.ascontiguousarray(pts[:, perm])
    b = _three(q, eps, mp)  # (border labels: only through the model of the permuted cloud)
    assert np.array_equal(b["count"], a["count"][perm]) and np.array_equal(b["core"], a["core"][perm])
    assert {frozenset(int(perm[k]) for k in g) for g in cm.core_partition(b)} == cm.core_partition(a)
    assert np.array_equal(b["labels"] < 0, a["labels"][perm] < 0)


def test_selection():
    # three clusters along a line, of 5, 9 and 5 points (a tie in size), and one stray
    t = np.concatenate([np.arange(5) * 0.01, 1.0 + np.arange(9) * 0.01, 2.0 + np.arange(5) * 0.01, [3.0]])
    pts = np.stack([t, 0 * t, 0 * t]).astype(np.float32)
    r = _three(pts, 0.011, 2)
    assert r["sizes"].tolist() == [5, 9, 5] and r["n_noise"] == 1 and r["n_out"] == 19
    assert _three(pts, 0.011, 2, min_size=6)["keep"].tolist() == [False] * 5 + [True] * 9 + [False] * 6
    assert _three(pts, 0.011, 2, min_size=0, max_size=5)["keep"].tolist() == [True] * 5 + [False] * 9 + [True] * 5 + [False]
    assert _three(pts, 0.011, 2, min_size=5, max_size=5)["n_out"] == 10
    assert _three(pts, 0.011, 2, min_size=10)["n_out"] == 0
    r = _three(pts, 0.011, 2, largest_only=True)
    assert r["keep"].tolist() == [False] * 5 + [True] * 9 + [False] * 6 and r["out_index"][5:14].tolist() == list(range(9))
    assert _three(pts, 0.011, 2, largest_only=True, max_size=5)["n_out"] == 0  # the largest of ALL clusters, then the bounds
    tie = np.ascontiguousarray(pts[:, [0, 1, 2, 3, 4, 14, 15, 16, 17, 18, 19]])  # 5 and 5: the lower label
    r = _three(tie, 0.011, 2, largest_only=True)
    assert r["sizes"].tolist() == [5, 5] and r["keep"].tolist() == [True] * 5 + [False] * 6
    assert _three(np.zeros((3, 0), np.float32), 0.1, 1, largest_only=True)["n_out"] == 0


def test_host_function_refusals_and_null_outputs():
    lib = binding.load()
    P = binding.ClusterParams
    pts = np.random.default_rng(2).uniform(0, 1, (3, 40)).astype(np.float32)
    none = [None] * 10

    def call(p, n=40, points=pts):
        return lib.icpk_cluster_host(None if points is None else binding._fp(points), n, None if p is None else C.byref(p), *none)

    good = P(0.2, 3, 1, 0, 0)
    assert call(good) == binding.OK and call(good, 0, None) == binding.OK
    bad = [P(0.0, 3, 1, 0, 0), P(-1.0, 3, 1, 0, 0), P(float("nan"), 3, 1, 0, 0), P(float("inf"), 3, 1, 0, 0), P(0.2, 0, 1, 0, 0),
           P(0.2, -2, 1, 0, 0), P(0.2, 3, -1, 0, 0), P(0.2, 3, 1, -1, 0), P(0.2, 3, 5, 4, 0), P(0.2, 3, 1, 0, 2), P(0.2, 3, 1, 0, -1)]
    for p in bad:
        assert call(p) == binding.E_ARG, list(bytes(p))
    assert call(None) == binding.E_ARG and call(good, -1) == binding.E_ARG and call(good, 40, None) == binding.E_ARG
    assert call(P(0.2, 3, 5, 5, 1)) == binding.OK and call(P(0.2, 3, 5, 0, 0)) == binding.OK
    nc, nn, no = C.c_int32(7), C.c_int32(7), C.c_int32(7)  # the counts are always initialised
    assert lib.icpk_cluster_host(binding._fp(pts), 40, C.byref(bad[0]), C.byref(nc), C.byref(nn), C.byref(no), *none[:7]) == binding.E_ARG
    assert (nc.value, nn.value, no.value) == (0, 0, 0)
    with pytest.raises(binding.IcpkError) as e:
        cluster.dbscan_host(pts, -1.0, 3)
    assert e.value.code == binding.E_ARG


def test_structure_layout():
    assert C.sizeof(binding.ClusterParams) == 20 and binding.ClusterParams.min_points.offset == 4
    assert binding.CLUSTER_LABELS_ONLY == 1


def test_clumps_of_strays_that_the_radius_filter_keeps():
    """Config 2's target plus 40 clumps of 12 points (sigma 4 mm), every centre more than 0.15 m from the surface and
    from the other centres: a clump's points have neighbours, so RADIUS (r = 0.05, min_neighbors = 5) keeps them, and a
    clump is a cluster of 12, so min_size = 50 removes it.  The plain target is two components at (0.05, 5)."""
    tgt = synth.kinect_pair()["target"]
    plain = cm.dbscan(tgt, 0.05, 5)
    print(f"config 2 target: {plain['n_clusters']} clusters of {plain['sizes'].tolist()}, border "
          f"{int(((plain['core'] == 0) & (plain['labels'] >= 0)).sum())}, noise {plain['n_noise']}")
    assert plain["n_clusters"] == 2 and plain["sizes"].sum() + plain["n_noise"] == tgt.shape[1]
    pts, stray = cm.with_clumps(tgt)
    assert int(stray.sum()) == 480
    rad = fm.remove_outliers(pts, fm.RADIUS, radius=0.05, min_neighbors=5)["keep"]
    got = cm.dbscan(pts, 0.05, 5, min_size=50)["keep"]
    s_rad, s_cl, g_cl = 1.0 - rad[stray].mean(), 1.0 - got[stray].mean(), 1.0 - got[~stray].mean()
    print(f"strays removed: RADIUS {100 * s_rad:.2f} %, clusters of >= 50 {100 * s_cl:.2f} %; genuine removed {100 * g_cl:.3f} %")
    assert s_rad < 0.05 and s_cl >= 0.95 and g_cl <= 0.001
