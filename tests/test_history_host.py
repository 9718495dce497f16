"""The history matrix on the host (tests/history_cases.py): the completeness table against binding.Context, the exempt
list, the scenes' determinism and sizes, and that the probe scene is sound for every model the matrix uses.

What the models find on P (asserted below; the figures are the ones the docstring of history_cases.py quotes):
  oracle.nn_bruteforce   the other target of the retarget probe changes the partner of 1641 of 1642 points;
                         1600 of 1642 first-sweep pairs lie within max_dist (0.12 m): the bound cuts pairs and keeps most
  robust_model           Huber, median scale, trim 0.9: 1440 of those 1600 kept
  gicp_model / color_model  the 28 sums of K5, K14 and K17 over 1600 accepted pairs
  normals_model          1697 of 1697 target and 1642 of 1642 source points get a normal (radius 0.25 m)
  voxel_model            698 target and 715 source voxels at a leaf of 0.15 m
  filter_model           statistical (k 8, 1 sigma) keeps 1438 / 1490, radius (0.2 m, 6) keeps 1633 / 1682
  color_model            930 of 1697 points get a gradient (the host normals are random unit vectors)
  score_model            1600, 1491, 1517, 1536 inliers at poses 0, 1, 2048, 4095
  fpfh_model             1642 + 1697 valid descriptors, 347 mutual matches, 15 of 64 hypotheses valid, the best with
                         1307 inliers (register_global ok); all 6000 hypotheses of the large run are valid
  tsdf_model             7424 and 7257 voxels updated by the two frames, 254 surface points
  tsdf_mesh_model        2828 triangles
  tsdf_raycast_model     152 hits from the source frame's pose
  map_model              1697 key points, 3164 voxels with a certainty
  fast_model             34 corners (7_12, suppressed), 219 (9_16, unsuppressed)
  posegraph_model        case A: 9 iterations to a cost of 0.080"""
import time

import numpy as np
import pytest

import history_cases as hc
from icp_slam_prototype_amd import binding

# the names that may be exempt, written out: methods that hold no device state of the context.  (tests/test_gpu_comm.py
# builds a communicator of one rank, so every RCCL call goes in as a history and none is exempt.)
EXEMPT = {"stream", "source_size", "target_size", "pair_distance", "set_log_callback", "close"}


def public_names():
    return {k for k in vars(binding.Context) if not k.startswith("_")}


def test_table_covers_the_class_exactly():
    names = public_names()
    assert len(names) > 100  # (the introspection sees the class, properties included)
    missing, stale = names - set(hc.COVERAGE), set(hc.COVERAGE) - names
    assert not missing, f"public names of binding.Context without a place in history_cases.COVERAGE: {sorted(missing)}"
    assert not stale, f"COVERAGE names that binding.Context no longer has: {sorted(stale)}"


def test_exempt_set_is_the_written_one():
    exempt = {k for k, v in hc.COVERAGE.items() if isinstance(v, hc.Exempt)}
    assert exempt == EXEMPT
    assert all(str(hc.COVERAGE[k]) for k in exempt)  # (each with its reason)


def source_of(user):
    """the text of a probe or early history with the text of every helper of history_cases it names, followed through
    (only those: a probe may not claim a call that a helper of another probe makes)"""
    import inspect
    import re

    from icp_slam_prototype_amd import batch

    helpers = {k: v for k, v in vars(hc).items() if inspect.isfunction(v) and v.__module__ == hc.__name__}
    helpers["RcclComm"] = batch.RcclComm
    fn = hc.PROBES.get(user) or hc.EARLY.get(user) or hc.SHARED[user]
    text = inspect.getsource(fn)
    if user in hc.PROBES and fn.__name__ == "probe":  # (made by make_nn_probe / make_align_probe: the enclosing maker)
        text = inspect.getsource(hc.make_nn_probe if user.startswith("nn_") else hc.make_align_probe)
    seen, todo = set(), [text]
    out = []
    while todo:
        t = todo.pop()
        out.append(t)
        for name in set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\(", t)) | set(re.findall(r"_quiet\((?:ctx\.)?([A-Za-z_]+)", t)):
            if name in helpers and name not in seen:
                seen.add(name)
                todo.append(inspect.getsource(helpers[name]))
    return "\n".join(out)


def test_every_entry_names_probes_or_histories_that_exist_and_call_it():
    import re

    known = set(hc.PROBES) | set(hc.EARLY) | set(hc.SHARED)
    source = {u: source_of(u) for u in known}
    for name, users in hc.COVERAGE.items():
        if isinstance(users, hc.Exempt):
            continue
        assert users and set(users) <= known, (name, users)
        for u in users:
            # the call itself, `.name(`, or the bound method handed to _quiet, `.name,` / `.name)`; a property: `.name` alone
            assert re.search(r"\.%s\b(?!_)" % re.escape(name), source[u]), f"{u} is listed for {name} and does not call it"
    # the check can fail: a probe that never touches the map is not a user of map_reset, and .align does not match
    # .align_batch
    assert not re.search(r"\.map_reset\b", source["nn_grid"])
    assert not re.search(r"\.align\b(?!_)", "ctx.align_batch(pairs)") and re.search(r"\.align\b(?!_)", "ctx.align(**kw)")


def test_histories_are_every_probe_on_q_and_s_and_the_early_paths():
    assert set(hc.HISTORIES) == {f"{s}.{p}" for s in "QS" for p in hc.PROBES} | set(hc.EARLY) | set(hc.SHARED)
    assert len(hc.PROBES) == 22 and len(hc.EARLY) == 12 and len(hc.SHARED) == 1
    assert set(hc.CHAIN_PROBES) == set(hc.PROBES) - {"tsdf", "map", "frontend", "batch", "posegraph"}
    assert set(hc.MODELS) == set(hc.PROBES) - {"batch"}


@pytest.mark.parametrize("name", ["P", "Q", "S"])
def test_scene_builders_are_deterministic(name):
    a, b = hc.build_scene(name), hc.build_scene(name)
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
        else:
            assert a[k] == b[k], k


def test_scene_sizes_sit_where_the_docstring_says():
    P, Q, S = hc.scene("P"), hc.scene("Q"), hc.scene("S")
    assert (P["source"].shape[1], P["target"].shape[1]) == (1642, 1697)
    assert (Q["source"].shape[1], Q["target"].shape[1]) == (3394, 3347)
    assert (S["source"].shape[1], S["target"].shape[1]) == (37, 37)
    for n in (1642, 1697):  # two tiles, the second partly filled; seven compaction workgroups, the last partly filled
        assert hc.NN_TILE < n < 2 * hc.NN_TILE and -(-n // hc.COMPACT_BLOCK) == 7 and n % hc.COMPACT_BLOCK
    for n in (3394, 3347):  # twice P: four tiles, every buffer grown past P's padded size (2 * NN_TILE)
        assert n > 2 * hc.NN_TILE and 1.8 < n / 1697 < 2.2 and -(-n // hc.NN_TILE) == 4
    assert 37 < hc.WAVE < hc.COMPACT_BLOCK < hc.NN_TILE
    # Q lies elsewhere and is larger: its bounding box does not contain P's and is more than 1.5 times as long
    lo_p, hi_p = P["target"].min(1), P["target"].max(1)
    lo_q, hi_q = Q["target"].min(1), Q["target"].max(1)
    assert ((hi_q - lo_q) > 1.5 * (hi_p - lo_p)).all() and (np.abs(lo_q - lo_p) > 1.0).any()
    # the constants the sizes are taken from are the code's
    import os
    import re

    csrc = os.path.join(os.path.dirname(binding.__file__), "csrc")
    with open(os.path.join(csrc, "icpk_internal.h")) as f:
        assert int(re.search(r"constexpr int NN_TILE = (\d+);", f.read()).group(1)) == hc.NN_TILE
    for kernels in ("kernels_voxel.hip", "kernels_filter.hip"):  # the cloud compactions' workgroup size
        with open(os.path.join(csrc, kernels)) as f:
            text = f.read()
        sizes = set(re.findall(r"block_total<(\d+)>", text)) | set(re.findall(r"block_excl_scan<(\d+)>", text))
        assert sizes == {str(hc.COMPACT_BLOCK)}, (kernels, sizes)
    for s in (P, Q, S):  # intensities in [0, 1], one per point; the depth frames give the clouds
        for side in ("source", "target"):
            v = s[side + "_intensity"]
            assert v.shape == (s[side].shape[1],) and v.min() >= 0 and v.max() <= 1
        assert int((s["depth_src"] != 0).sum()) == s["source"].shape[1]


@pytest.fixture(scope="module")
def facts(oracle):
    """every model of the matrix run on P once; (facts per probe, seconds per probe)"""
    s = hc.scene("P")
    out, took = {}, {}
    for k, m in hc.MODELS.items():
        t0 = time.time()
        out[k] = m(s, oracle)["facts"]
        took[k] = time.time() - t0
    return out, took


def test_p_is_sound_for_every_model(facts):
    f, took = facts
    print({k: round(v, 2) for k, v in took.items()})
    assert max(took.values()) < 20 and sum(took.values()) < 60  # (seconds; the whole of it takes about ten)
    n_s, n_t = 1642, 1697
    assert f["retarget"]["changed"] > n_s / 2                               # the other target changes most partners
    assert 0.9 * n_s < f["nn_grid"]["near"] < n_s                        # the distance bound cuts pairs, keeps most
    for k in ("point_to_plane", "plane_to_plane", "colored"):
        assert f["align_" + k]["accepted"] > 0.9 * n_s
    assert 0.8 * n_s < f["align_robust"]["kept"] < f["align_robust"]["accepted"]  # the trim does cut
    assert f["normals"]["target_valid"] > n_t / 2 and f["normals"]["source_valid"] > n_s / 2
    assert 100 < f["voxel"]["target_out"] < n_t / 2 and 100 < f["voxel"]["source_out"] < n_s / 2
    for key, (n_in, n_out) in f["filter"].items():
        assert n_in / 2 < n_out < n_in, key                               # each filter removes points, none removes most
    assert f["color"]["with_gradient"] > n_t / 2
    assert all(n_s / 2 < k <= n_s for k in f["score"]["inliers"]) and len(set(f["score"]["inliers"])) > 1
    g = f["fpfh"]
    assert g["matches"] >= 10 and g["ok"] and g["inliers"] > n_s / 2 and g["n_valid"] >= 3 and min(g["valid"]) > n_s / 2
    t = f["tsdf"]
    assert min(t["updated"]) > 1000 and t["surface"] > 100 and t["triangles"] > 100 and t["hits"] > 50
    assert f["map"]["keypoints"] > 1000 and f["map"]["voxels"] > 1000
    assert f["frontend"]["corners"] >= 20 and f["frontend"]["corners916"] >= 20
    assert f["posegraph"]["iterations"] >= 3 and f["posegraph"]["final_cost"] > 0


def test_probe_figures_match_the_docstring(facts):
    """the counts the module's docstring states (a changed scene or setting shows here first)"""
    f, _ = facts
    assert f["nn_grid"]["near"] == 1600 and f["align_robust"] == dict(accepted=1600, kept=1440)
    assert f["normals"] == dict(n=1697, target_valid=1697, source_valid=1642)
    assert f["voxel"] == dict(target_out=698, source_out=715)
    assert f["filter"] == {"statistical.0": (1642, 1438), "statistical.1": (1697, 1490), "radius.0": (1642, 1633),
                           "radius.1": (1697, 1682)}
    assert f["color"]["with_gradient"] == 930 and f["score"]["inliers"] == [1600, 1491, 1517, 1536]
    assert (f["fpfh"]["matches"], f["fpfh"]["n_valid"], f["fpfh"]["inliers"]) == (347, 15, 1307)
    assert f["fpfh"]["large_n_valid"] == 6000 > binding.SCORE_MAX_POSES  # the large run crosses a scoring chunk
    assert f["tsdf"] == dict(updated=[7424, 7257], surface=254, triangles=2828, hits=152)
    assert (f["map"]["keypoints"], f["map"]["voxels"]) == (1697, 3164)
    assert f["frontend"] == dict(corners=34, corners916=219)


def test_first_difference_names_the_element():
    a = hc.blob(np.arange(6, dtype=np.float32).reshape(2, 3))
    b = np.arange(6, dtype=np.float32).reshape(2, 3)
    b[1, 1] = 9
    msg = hc.first_difference(a, hc.blob(b))
    assert "flat index 4" in msg and "1 of 6" in msg
    assert "bytes against" in hc.first_difference(a, hc.blob(b[:1]))
    assert hc.unblob(a).tobytes() == a and hc.unblob(a).shape == (2, 3)
