"""The history matrix of the image and volume families on the host (tests/history_image_cases.py): the completeness
table against the functions over a context of binding.py and depth.py, the scenes' and volumes' determinism and sizes,
that P and Q are sound for every probe, and every expected byte by two routes -- the numpy model and the library's
host-only rule function.

The figures the models give (asserted below; they are the ones history_image_cases.py's docstring quotes) are written
out in test_probe_figures_match_the_docstring.

The two routes compare bit for bit throughout: each family's own host test claims bit equality between its model and
its host rule function (tests/test_bilateral_host.py, test_pyramid_host.py, test_projective_host.py,
test_projective_color_host.py, test_frame_view_host.py, test_esdf_host.py, and for the TSDF rules
tests/test_gpu_tsdf*.py's host halves), so no tolerance is taken from anywhere."""
import inspect
import re
import types

import numpy as np
import pytest

import history_cases as hc
import history_image_cases as hi
import thread_cases
from icp_slam_prototype_amd import binding, depth

B, D = binding, depth
F32 = np.float32

# an exemption needs a written reason: name -> reason.  The ten fern functions (K27) are exempt: the probe written for them
# faulted on the GPU once, the cause was not found, and probe, histories and tests were taken out together.
FERN_NAMES = ("fern_create", "fern_reset", "fern_destroy", "fern_count", "fern_encode", "fern_query", "fern_add", "fern_process",
              "fern_add_code", "fern_keyframe")
EXEMPT = {k: hi._FERN_LEFT_OUT for k in FERN_NAMES}


# ------------------------------------------------------------------------------------------------------ the table --
def context_functions(*modules):
    """the public module-level functions whose first parameter is named `ctx`"""
    out = {}
    for m in modules:
        for k, v in vars(m).items():
            if k.startswith("_") or not inspect.isfunction(v) or v.__module__ != m.__name__:
                continue
            params = list(inspect.signature(v).parameters)
            if params and params[0] == "ctx":
                out[k] = v
    return out


def table_gaps(names, coverage):
    """(names without a place, places without a name)"""
    return sorted(set(names) - set(coverage)), sorted(set(coverage) - set(names))


def source_of(user, cases=hi):
    """the text of a probe or early history with the text of every helper of history_image_cases it names, followed
    through (as tests/test_history_host.py::source_of does for history_cases)"""
    helpers = {k: v for k, v in vars(cases).items() if inspect.isfunction(v) and v.__module__ == cases.__name__}
    fn = cases.PROBES.get(user) or cases.EARLY[user]
    seen, todo, out = {fn.__name__}, [inspect.getsource(fn)], []
    while todo:
        t = todo.pop()
        out.append(t)
        for name in set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\(", t)):
            if name in helpers and name not in seen:
                seen.add(name)
                todo.append(inspect.getsource(helpers[name]))
    return "\n".join(out)


def calls(name, text):
    """the call itself, `B.name(` / `D.name(`, or the function handed on, `B.name,` / `B.name)`"""
    return re.search(r"\b[BD]\.%s\b(?!_)" % re.escape(name), text) is not None


def users_that_do_not_call(coverage, cases=hi):
    known = set(cases.OWN_PROBES) | set(cases.EARLY)
    source = {u: source_of(u, cases) for u in known}
    bad = []
    for name, users in coverage.items():
        if isinstance(users, hc.Exempt):
            continue
        if not users or not set(users) <= known:
            bad.append((name, "unknown users", tuple(users)))
            continue
        bad += [(name, "is not called by", u) for u in users if not calls(name, source[u])]
    return bad


def test_table_covers_the_functions_exactly():
    names = context_functions(binding, depth)
    missing, stale = table_gaps(names, hi.COVERAGE)
    assert not missing, f"functions over a context without a place in history_image_cases.COVERAGE: {missing}"
    assert not stale, f"COVERAGE names that are no function over a context: {stale}"
    # (the introspection sees what the table was written for: 43 functions of binding.py, tsdf_shift to esdf_release, 6 of depth.py)
    assert len(names) == 49 and len(context_functions(binding)) == 43 and len(context_functions(depth)) == 6
    first, last = list(context_functions(binding))[0], list(context_functions(binding))[-1]
    assert (first, last) == ("tsdf_shift", "esdf_release")
    assert not [k for k in names if hasattr(binding.Context, k)]  # (none of them is a method as well)
    assert set(thread_cases.MODULE_FUNCTIONS) <= set(hi.COVERAGE)
    for k, fn in thread_cases.MODULE_FUNCTIONS.items():
        assert names[k] is fn


def test_exempt_set_is_the_written_one():
    exempt = {k: str(v) for k, v in hi.COVERAGE.items() if isinstance(v, hc.Exempt)}
    assert exempt == EXEMPT and len(exempt) == 10 and "faulted" in hi._FERN_LEFT_OUT
    assert all(reason.strip() for reason in exempt.values())


def test_every_entry_names_users_that_exist_and_call_it():
    assert not users_that_do_not_call(hi.COVERAGE)
    # every probe of the nine is somebody's user, and every early history too
    used = {u for users in hi.COVERAGE.values() for u in users}
    assert set(hi.OWN_PROBES) <= used
    # (early_image_refusals is nobody's user: a refused call installs nothing; it is a history all the same)
    assert set(hi.EARLY) - used == {"early_image_refusals"}


def test_the_table_test_can_fail():
    """a function over a context added later has no place; a listed user that stops calling its function is found"""
    later = types.ModuleType("later")
    exec("def something(ctx):\n    return ctx\n\ndef _private(ctx):\n    pass\n\ndef other(points, ctx):\n    pass\n", later.__dict__)
    for f in ("something", "_private", "other"):
        getattr(later, f).__module__ = "later"
    names = dict(context_functions(binding, depth), **context_functions(later))
    assert list(context_functions(later)) == ["something"]  # (not the private one, not one whose ctx comes second)
    assert table_gaps(names, hi.COVERAGE) == (["something"], [])
    assert table_gaps(context_functions(binding), hi.COVERAGE)[1] == sorted(context_functions(depth))
    # `esdf` does not shift the volume, and `bilateral` never builds a pyramid: listed there, both are found
    wrong = dict(hi.COVERAGE, tsdf_shift=("esdf",), build_pyramid=("bilateral",))
    assert sorted(users_that_do_not_call(wrong)) == [("build_pyramid", "is not called by", "bilateral"),
                                                     ("tsdf_shift", "is not called by", "esdf")]
    assert users_that_do_not_call(dict(hi.COVERAGE, tsdf_shift=("no_such_probe",)))
    # the pattern tells a name from the names it is a prefix of
    assert calls("esdf_get", "B.esdf_get(ctx)") and not calls("esdf_get", "B.esdf_get_box(ctx, lo, hi)")
    assert calls("frame_view", "_quiet(B.frame_view, ctx, 0)") and not calls("frame_view", "B.frame_view_build(ctx, P)")
    assert calls("build_pyramid", "D.build_pyramid(ctx, d)") and not calls("build_pyramid", "build_pyramid(ctx, d)")


def test_histories_are_every_probe_on_q_and_s_the_old_ones_on_q_and_the_early_paths():
    own = {f"{s}.{p}" for s in "QS" for p in hi.OWN_PROBES if not (s == "S" and p in hi.S_REFUSED)}
    assert set(hi.HISTORIES) == own | {f"Q.old.{p}" for p in hi.OLD_ON_Q} | set(hi.EARLY)
    assert len(hi.OWN_PROBES) == 9 and len(own) == 18 - len(hi.S_REFUSED) and len(hi.S_REFUSED) <= 2
    assert set(hi.OLD_ON_Q) == {"tsdf", "frontend", "align_point_to_plane"} and len(hi.EARLY) == 11
    assert set(hi.PROBE_ORDER) == set(hi.OWN_PROBES) | {"tsdf", "frontend"} and len(hi.PROBE_ORDER) == 11
    assert hi.PROBES["tsdf"] is hc.PROBES["tsdf"] and hi.PROBES["frontend"] is hc.PROBES["frontend"]
    assert set(hi.MODELS) == set(hi.PROBES) and hi.CHAIN == "QSPSQP"


# ------------------------------------------------------------------------------------- scenes, volumes, inputs --
@pytest.mark.parametrize("name", ["P", "Q", "S"])
def test_inputs_are_deterministic_across_two_builds(name):
    a, b = hc.build_scene(name), hc.build_scene(name)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
        else:
            assert a[k] == b[k], k
    assert a["depth_src"].tobytes() == hi.scene(name)["depth_src"].tobytes()
    pts = hi.query_points(hi.scene(name))
    hi._query_points_cached.cache_clear()
    assert pts.tobytes() == hi.query_points(hi.scene(name)).tobytes()


def test_scene_and_volume_sizes():
    P, Q, S = (hi.scene(k) for k in "PQS")
    assert (P["rows"], P["cols"]) == (40, 60) and (Q["rows"], Q["cols"]) == (60, 80) and (S["rows"], S["cols"]) == (6, 8)
    assert hi.VOLUMES["P"] is hc.TSDF_VOLUME and hi.VOLUMES["P"]["dims"] == (33, 31, 29)
    n = {k: hi.voxels(k) for k in "PQS"}
    assert n == dict(P=29667, Q=79335, S=60) and max(n.values()) < 10 ** 5
    assert n["Q"] > n["P"] and all(d % 2 for d in hi.VOLUMES["Q"]["dims"])
    assert hi.VOLUMES["Q"]["voxel"] != hi.VOLUMES["P"]["voxel"] and hi.VOLUMES["Q"]["origin"] != hi.VOLUMES["P"]["origin"]
    assert n["S"] < hi.TSDF_THREADS and max(hi.VOLUMES["S"]["dims"]) <= 5
    # every level of every pyramid a probe builds has a pixel, every box a voxel: no probe's shapes are refused on S
    for s in (P, Q, S):
        assert all(r >= 1 and c >= 1 for r, c in D.pyramid_shapes((s["rows"], s["cols"]), hi.SMOOTH_PYRAMID["levels"]))
        for lo, hi_ in (hi.follow_box(s["name"]), hi.esdf_box(s["name"])):
            assert all(0 <= a < b <= d for a, b, d in zip(lo, hi_, hi.VOLUMES[s["name"]]["dims"]))
        assert min(hi.VOLUMES[s["name"]]["dims"]) >= 2  # (a dim of 1 has no cell for the query and the ray rule)


def test_the_three_volumes_differ_in_their_chunks():
    """The chunk rule, restated: chunk = max(256, ceil(ceil(n / 8192) / 256) * 256) voxels, ceil(n / chunk) chunks.  Below
    256 * 8192 voxels the LENGTH is 256 whatever the volume, so three volumes under 10^5 voxels -- P is fixed at 29 667,
    S at a few voxels per side -- cannot differ in it; they differ in the NUMBER of chunks, which sizes every per-chunk
    buffer (the slots, the mesh's per-chunk counts and offsets, the distance map's counts), and P's and Q's last chunks
    are partly filled at different lengths."""
    import os

    with open(os.path.join(os.path.dirname(binding.__file__), "csrc", "icpk_internal.h")) as f:
        text = f.read()
    assert int(re.search(r"constexpr int TSDF_THREADS = (\d+);", text).group(1)) == hi.TSDF_THREADS
    assert int(re.search(r"constexpr int TSDF_MAX_BLOCKS = (\d+);", text).group(1)) == hi.TSDF_MAX_BLOCKS
    assert "const long long per = (n + TSDF_MAX_BLOCKS - 1) / TSDF_MAX_BLOCKS;" in text
    assert "const long long c = (per + TSDF_THREADS - 1) / TSDF_THREADS * TSDF_THREADS;" in text
    assert [hi.chunk_length(n) for n in (1, 256, 257, 256 * 8192, 256 * 8192 + 1, 2 ** 30)] == [256, 256, 256, 256, 512, 131072]
    n = {k: hi.voxels(k) for k in "PQS"}
    assert {k: hi.chunk_length(v) for k, v in n.items()} == dict(P=256, Q=256, S=256)
    counts = {k: hi.chunk_count(v) for k, v in n.items()}
    assert counts == dict(P=116, Q=310, S=1) and len(set(counts.values())) == 3
    tails = {k: v % 256 for k, v in n.items()}
    assert tails == dict(P=227, Q=231, S=60) and len(set(tails.values())) == 3 and all(tails.values())


# --------------------------------------------------------------------------------------------------- soundness --
@pytest.fixture(scope="module")
def models():
    """every model of the nine probes on P, Q and S, once"""
    return {n: {k: hi.MODELS[k](hi.scene(n)) for k in hi.OWN_PROBES} for n in "PQS"}


MIN_PAIRS = 6  # what every loop of the probes asks for (projective_params, sdf_params)


@pytest.mark.parametrize("name", ["P", "Q"])
def test_scene_is_sound_for_every_probe(models, name):
    f = {k: v["facts"] for k, v in models[name].items()}
    s = hi.scene(name)
    npix = s["rows"] * s["cols"]
    assert 0 < f["bilateral"]["changed"] <= f["bilateral"]["valid"] < npix       # the filter changes pixels, holes stay
    assert all(v > 0 for v in f["pyramid"]["valid"] + f["pyramid"]["smooth_valid"])
    v = f["volume_follow"]
    assert min(v["updated"]) > 1000
    assert v["leaving"] >= 1 and v["kept"] >= 1 and v["leaving"] + v["kept"] == v["before"]  # the shift streams out and keeps
    assert v["after"] > 100 and v["triangles"] > 100 and v["hits"] > 50
    a = f["volume_apply"]
    assert min(a["counts"]) > 1000 and a["deintegrate"] > 1000 and a["resident"] > 1000
    assert a["cancelling"][0] == a["cancelling"][1] >= 1 and a["left"] == 0         # the cancelling ops touch voxels
    # every loop accepts at least its minimum count at iteration 0
    assert min(f["projective"]["pairs"]) >= MIN_PAIRS and f["projective"]["hits"] > 50
    assert min(f["projective_colored"]["pairs"]) >= MIN_PAIRS and f["projective_colored"]["with_gradient"] >= MIN_PAIRS
    w = f["frame_view"]
    assert min(w["pairs"]) >= MIN_PAIRS and min(w["listed"]) > 0 and min(w["plain_listed"]) > 0 and w["colored"] and w["uncoloured"]
    assert min(f["sdf"]["accepted"]) >= MIN_PAIRS
    e = f["esdf"]
    assert e["R"] == hi.ESDF_RADIUS and min(e["counts"][:3]) > 0                    # all three classes
    assert e["outside"] > 0 and e["inside"] > 0 and e["outside"] + e["inside"] == e["points"]


def test_the_tiny_scene_refuses_no_probe(models):
    """the models run to their end on S: what the probes meet there are statuses (no pair, no crossing), not refusals.
    What the header refuses by shape -- a level without a pixel, an empty box, a radius below one voxel -- does not
    occur (test_scene_and_volume_sizes), so S_REFUSED is empty."""
    f = {k: v["facts"] for k, v in models["S"].items()}
    assert hi.S_REFUSED == () and f["esdf"]["R"] == hi.ESDF_RADIUS >= 1
    assert f["projective"]["pairs"] == [0, 0] and f["sdf"]["accepted"] == [0, 0, 0]  # the loops end with W_TOO_FEW_PAIRS
    assert f["volume_follow"]["before"] == 0 and f["volume_apply"]["left"] == 0
    # the docstring's figures for S
    assert f["volume_follow"] == dict(updated=[31, 32], before=0, leaving=0, kept=0, after=0, triangles=12, hits=0)
    assert f["projective_colored"] == dict(with_gradient=0, pairs=[0, 0]) and f["frame_view"]["pairs"] == [6, 0]


def test_probe_figures_match_the_docstring(models):
    """the counts the module's docstring states (a changed scene or setting shows here first)"""
    p, q = ({k: v["facts"] for k, v in models[n].items()} for n in "PQ")
    assert p["bilateral"] == dict(changed=1543, valid=1642) and q["bilateral"] == dict(changed=3191, valid=3394)
    assert p["pyramid"] == dict(valid=[1642, 409, 99], smooth_valid=[1697, 432, 109, 26])
    assert p["volume_follow"] == dict(updated=[7424, 7257], before=254, leaving=30, kept=224, after=248, triangles=2806, hits=142)
    assert q["volume_follow"] == dict(updated=[16156, 16297], before=877, leaving=29, kept=848, after=909, triangles=7114, hits=295)
    assert p["volume_apply"] == dict(counts=[7424, 7257, 7264, 7257, 7438, 7424], deintegrate=7264, resident=7257,
                                     cancelling=[7424, 7424], left=0)
    assert p["projective"] == dict(hits=152, pairs=[104, 29]) and q["projective"] == dict(hits=292, pairs=[229, 63])
    assert p["projective_colored"] == dict(with_gradient=35, pairs=[104, 29]) and q["projective_colored"]["with_gradient"] == 72
    assert (p["frame_view"]["listed"], p["frame_view"]["plain_listed"], p["frame_view"]["pairs"]) == ([334, 64, 18], [397, 111, 17], [220, 50])
    assert (q["frame_view"]["listed"], q["frame_view"]["plain_listed"], q["frame_view"]["pairs"]) == ([814, 167, 66], [717, 141, 25], [547, 113])
    assert p["sdf"] == dict(accepted=[590, 149, 540]) and q["sdf"] == dict(accepted=[1486, 385, 1311])
    assert p["esdf"] == dict(R=4, counts=[20021, 7679, 1967, 22423], points=112, outside=38, inside=74, clean=3)
    assert (q["esdf"]["counts"], q["esdf"]["outside"], q["esdf"]["inside"]) == ([57873, 17596, 3866, 59904], 39, 73)


# ---------------------------------------------------------------------------------- the expected bytes, two routes --
def same(got, want, key):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != want.dtype and got.dtype.kind in "iub" and want.dtype.kind in "iub":
        assert np.array_equal(got, want), key
        return
    assert got.dtype == want.dtype and got.shape == want.shape, (key, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), f"{key}: {hc.first_difference(hc.blob(got), hc.blob(want))}"


def volume_params(name, origin=None, color=True):
    v = hi.VOLUMES[name]
    return B.tsdf_params(dims=v["dims"], voxel=v["voxel"], origin=v["origin"] if origin is None else [float(x) for x in origin],
                         trunc=v["trunc"], flags=B.TSDF_COLOR if color else 0)


def host_fuse(s, params, planes):
    """icpk_tsdf_voxel_update for the scene's two frames over (tsdf, weight, intensity), in place; the voxels written"""
    n = []
    for d, P, img in hi._frames(s):
        R, t = B.tsdf_invert_pose(P)
        n.append(B.tsdf_voxel_update(params, R, t, d, planes[0].reshape(-1), planes[1].reshape(-1), img, planes[2].reshape(-1),
                                     fx=s["fx"], cx=s["cx"]))
    return n


def host_raycast(s, params, planes):
    ray = B.tsdf_raycast_params(shape=(s["rows"], s["cols"]), fx=s["fx"], cx=s["cx"], **hi.RAY_VIEW)
    maps, n = B.tsdf_raycast_pixels(params, ray, s["pose_src"], *planes)
    return maps.reshape(8, s["rows"], s["cols"]), n


def host_projective(s, l, a, colored=None):
    """icpk_projective_pixels (colored: icpk_projective_pixels_colored) for the arguments of the model's pixels"""
    p = hi.projective_params(s, l)
    if a["view_shape"] == (s["rows"], s["cols"]) and a["fx_v"] == s["fx"]:
        view_fx, view_cx = s["fx"], s["cx"]       # the ray cast's camera
    else:
        view_fx, view_cx = hi.level_camera(s, l)  # the frame view's level
    args = (p, a["pose"], a["level"], a["view"], a["view_shape"], float(view_fx), float(view_cx), a["view_pose"])
    if colored is None:
        return B.projective_pixels(*args, terms=True)
    return B.projective_pixels_colored(*args, colored["level_intensity"], colored["gradient"],
                                       color=dict(lambda_geometric=hi.LAMBDA), terms=True)


def check_pixels(model, key, shape, host, reduce):
    pixel, dist, terms, n = host
    same(pixel.reshape(shape), model[key + ".pixel"], key + ".pixel") if key + ".pixel" in model else None
    same(dist.reshape(shape), model[key + ".dist"], key + ".dist") if key + ".dist" in model else None
    return reduce(terms, pixel), n


@pytest.fixture(scope="module")
def p_models(models):
    return models["P"]


def test_two_routes_bilateral_and_pyramid(p_models):
    s = hi.scene("P")
    m = p_models["bilateral"]
    p = D.bilateral_params(**hi.BILATERAL)
    same(D.bilateral_host(s["depth_src"], p), m["smooth"], "smooth")
    same(D.bilateral_host(s["depth_tgt"]), m["smooth_default"], "smooth_default")
    same(D.bilateral_host(s["depth_tgt"], p), m["in_place"], "in_place")
    m = p_models["pyramid"]
    smoothed = D.bilateral_host(s["depth_tgt"], p)
    for tag, img, inten, kw in (("plain", s["depth_src"], s["image_src"], hi.PYRAMID), ("smooth", smoothed, s["image_tgt"], hi.SMOOTH_PYRAMID)):
        pp = D.pyramid_params(**kw)
        for l in range(kw["levels"]):
            same(D.pyramid_host(img, l, pp), m[f"{tag}.level{l}"], f"{tag}.level{l}")
            same(B.intensity_pyramid_host(img, inten, l, pp), m[f"{tag}.intensity{l}"], f"{tag}.intensity{l}")
            same(np.array(D.pyramid_shapes(img.shape, kw["levels"])[l]), m[f"{tag}.shape{l}"], f"{tag}.shape{l}")


def test_two_routes_volume_follow(p_models):
    import tsdf_shift_model as shm

    s = hi.scene("P")
    m = p_models["volume_follow"]
    base, _ = hi.fused("P")
    planes = [np.zeros_like(base.tsdf), np.zeros_like(base.weight), np.zeros_like(base.intensity)]
    same(host_fuse(s, volume_params("P"), planes), m["n_updated"], "n_updated")
    for got, want in zip(planes, (base.tsdf, base.weight, base.intensity)):
        same(got, want, "the fused planes")
    moved = shm.shifted(base, hi.SHIFT)
    params = volume_params("P", origin=moved.origin)
    same(np.array(params.origin[:], F32), m["shifted.origin"], "shifted.origin")
    planes = [moved.tsdf.copy(), moved.weight.copy(), moved.intensity.copy()]
    same(host_fuse(s, params, planes), m["n_updated_again"], "n_updated_again")
    for k, a in zip(("tsdf", "weight", "intensity"), planes):
        same(a, m["planes." + k], "planes." + k)
    maps, n = host_raycast(s, params, planes)
    same(maps, m["raycast.maps"], "raycast.maps")
    assert n == m["raycast.counts"][0]
    mesh = B.tsdf_mesh_host(params, *planes, min_weight=1)
    for k in ("vertices", "normals", "intensity", "voxel_index", "edge", "triangles"):
        same(mesh[k], m["mesh." + k], "mesh." + k)
    assert [mesh["n_vertices"], mesh["n_triangles"], mesh["n_no_normal"]] == m["mesh.counts"].tolist()


def test_two_routes_volume_apply(p_models):
    s = hi.scene("P")
    m = p_models["volume_apply"]
    params = volume_params("P")
    n = hi.voxels("P")
    f, w, c = np.zeros(n, F32), np.zeros(n, np.uint16), np.zeros(n, F32)
    frames, images = [s["depth_tgt"], s["depth_src"]], [s["image_tgt"], s["image_src"]]
    kw = dict(intensities=images, intensity_value=c, fx=s["fx"], cx=s["cx"])

    def planes(key):
        for k, a in (("tsdf", f), ("weight", w), ("intensity", c)):
            same(a.reshape(m[f"{key}.{k}"].shape), m[f"{key}.{k}"], f"{key}.{k}")

    same(B.tsdf_voxel_apply(params, frames, hi.apply_ops(s), f, w, **kw), m["apply.counts"], "apply.counts")
    planes("apply")
    one = B.tsdf_voxel_apply(params, [s["depth_src"]], [(-1, 0, hi.drift(s["pose_src"]))], f, w, intensities=[s["image_src"]],
                             intensity_value=c, fx=s["fx"], cx=s["cx"])
    same(one[0], m["deintegrate.count"], "deintegrate.count")
    planes("deintegrate")
    R, t = B.tsdf_invert_pose(s["pose_src"])
    k = B.tsdf_voxel_update(params, R, t, s["depth_src"], f, w, s["image_src"], c, fx=s["fx"], cx=s["cx"])
    assert k == m["resident.count"]
    planes("resident")
    f, w, c = np.zeros(n, F32), np.zeros(n, np.uint16), np.zeros(n, F32)
    counts = B.tsdf_voxel_apply(params, frames, hi.cancelling_ops(s), f, w, intensities=images, intensity_value=c, fx=s["fx"], cx=s["cx"])
    assert counts.tolist() == m["facts"]["cancelling"] and not f.any() and not w.any() and not c.any()


def test_two_routes_projective_and_colored(p_models):
    import projective_color_model as qm
    import projective_model as jm

    s = hi.scene("P")
    base, _ = hi.fused("P")
    maps, n = host_raycast(s, volume_params("P"), (base.tsdf, base.weight, base.intensity))
    m, mc = p_models["projective"], p_models["projective_colored"]
    same(maps, m["raycast.maps"], "raycast.maps")
    assert n == m["raycast.counts"][0] == mc["raycast.counts"][0]
    S, g, with_gradient = B.raycast_color_gradients_host(maps, hi.GRADIENT_RADIUS, hi.GRADIENT_MIN_NB)
    gradient = np.ascontiguousarray(g.T).reshape(3, s["rows"], s["cols"])
    same(gradient, mc["gradients"], "gradients")
    same(S.reshape(s["rows"], s["cols"], 10), mc["gradient_sums"], "gradient_sums")
    assert with_gradient == mc["facts"]["with_gradient"]
    for l in (0, 1):
        a = hi.projective_args(s, l)
        shape = a["level"].shape
        (sums, count), pairs = check_pixels(m, f"l{l}", shape, host_projective(s, l, a), jm.reduce)
        same(sums, m[f"l{l}.sums"], f"l{l}.sums")
        assert count == pairs == m[f"l{l}.count"]
        inten = B.intensity_pyramid_host(s["depth_src"], s["image_src"], l, D.pyramid_params(**hi.PYRAMID))
        same(inten, mc[f"l{l}.intensity"], f"l{l}.intensity")
        host = host_projective(s, l, a, dict(level_intensity=inten, gradient=gradient))
        (sums, count), pairs = check_pixels(m, f"l{l}", shape, host, qm.reduce)  # (the coloured path pairs as K25 does)
        same(sums, mc[f"l{l}.colored.sums"], f"l{l}.colored.sums")
        assert count == pairs == mc[f"l{l}.colored.count"]


def test_two_routes_frame_view(p_models):
    import projective_color_model as qm
    import projective_model as jm

    s = hi.scene("P")
    m = p_models["frame_view"]
    pp = D.pyramid_params(**hi.PYRAMID)
    for tag, which, color in (("plain", "tgt", False), ("color", "src", True)):
        counts = []
        for l in range(hi.PYRAMID["levels"]):
            img = D.pyramid_host(s["depth_" + which], l, pp)
            inten = B.intensity_pyramid_host(s["depth_" + which], s["image_" + which], l, pp) if color else None
            planes, n_valid, n_none = B.frame_view_pixels(img, s["pose_" + which], fx=s["fx"], cx=s["cx"], level=l, intensity=inten)
            same(planes.reshape(8, *img.shape), m[f"{tag}.planes{l}"], f"{tag}.planes{l}")
            counts.append((n_valid, n_none))
        same(np.array(counts, np.int32).T, m[tag + ".counts"], tag + ".counts")
    est = hi.drift(s["pose_tgt"])
    for l in (0, 1):
        view = m[f"color.planes{l}"]
        S, g, _ = B.raycast_color_gradients_host(view, hi.GRADIENT_RADIUS * 2 ** l, hi.GRADIENT_MIN_NB)
        gradient = np.ascontiguousarray(g.T).reshape(3, *view.shape[1:])
        same(gradient, m[f"color.gradients{l}"], f"color.gradients{l}")
        a = hi.projective_args(s, l, "tgt", view=view, view_pose=s["pose_src"], estimate=est)
        shape = a["level"].shape
        (sums, count), pairs = check_pixels(m, f"view.l{l}", shape, host_projective(s, l, a), jm.reduce)
        same(sums, m[f"view.l{l}.sums"], f"view.l{l}.sums")
        assert count == pairs == m[f"view.l{l}.count"]
        inten = B.intensity_pyramid_host(s["depth_tgt"], s["image_tgt"], l, pp)
        host = host_projective(s, l, a, dict(level_intensity=inten, gradient=gradient))
        (sums, count), pairs = check_pixels(m, f"view.l{l}", shape, host, qm.reduce)
        same(sums, m[f"view.l{l}.colored.sums"], f"view.l{l}.colored.sums")
        assert count == pairs == m[f"view.l{l}.colored.count"]


def test_two_routes_sdf(p_models):
    import sdf_track_model as sm
    import tsdf_shift_model as shm

    s = hi.scene("P")
    m = p_models["sdf"]
    base, _ = hi.fused("P")
    moved = shm.shifted(base, hi.SHIFT)
    est = hi.drift(s["pose_src"])
    pp = D.pyramid_params(**hi.PYRAMID)
    for key, vol, levels in (("fused", base, (0, 1)), ("shifted", moved, (0,))):
        params = volume_params("P", origin=vol.origin, color=False)
        for l in levels:
            img = D.pyramid_host(s["depth_src"], l, pp)
            cell, value, terms, n = B.sdf_pixels(hi.sdf_params(s, l), params, est, img, vol.tsdf, vol.weight, terms=True)
            same(cell.reshape(img.shape), m[f"{key}.l{l}.cell"], f"{key}.l{l}.cell")
            same(value.reshape(img.shape), m[f"{key}.l{l}.value"], f"{key}.l{l}.value")
            sums, count = sm.reduce(terms, cell)
            same(sums, m[f"{key}.l{l}.sums"], f"{key}.l{l}.sums")
            assert count == n == m[f"{key}.l{l}.count"]


def test_two_routes_esdf(p_models):
    s = hi.scene("P")
    m = p_models["esdf"]
    base, _ = hi.fused("P")
    params = volume_params("P", color=False)
    sq, cls, dist, counts = B.esdf_host(params, base.tsdf, base.weight, **hi.esdf_kw(s))
    for k, a in (("sq", sq), ("cls", cls), ("dist", dist), ("counts", counts)):
        same(a, m[k], k)
    q = B.esdf_query_host(params, sq, cls, hi.query_points(s), **hi.esdf_kw(s))
    for k, a in q.items():
        same(a, m["query." + k], "query." + k)
    st = q["status"]
    assert (st == B.ESDF_Q_OUTSIDE).sum() == m["facts"]["outside"] and st[-1] == B.ESDF_Q_OUTSIDE  # (the NaN point)
