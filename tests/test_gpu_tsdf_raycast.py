"""The ray cast of the TSDF volume on the device (K20; icpk_tsdf_raycast*) against tests/tsdf_raycast_model.py, bit for
bit: the eight maps and both counts on every case of the table, the hand-over as the context's target, what the calls
leave alone, every refusal the header names, and tsdf.ModelTracker over the room frames."""
import numpy as np
import pytest

import tsdf_cases as tc
import tsdf_model
import tsdf_raycast_cases as rc
import tsdf_raycast_model as rm
from icp_slam_prototype_amd import binding, synth
from icp_slam_prototype_amd.tsdf import ModelTracker, TsdfVolume

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with binding.Context(0) as c:
        yield c


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def fuse(ctx, case):
    """the case's volume on the context, with its frames"""
    c = tc.case(case)
    v = c["volume"]
    ctx.tsdf_create(dims=v["dims"], voxel=v["voxel"], origin=v["origin"], trunc=v["trunc"], max_weight=v.get("max_weight"),
                    flags=binding.TSDF_COLOR if v.get("color") else 0)
    for d, P, img in c["frames"]:
        ctx.tsdf_integrate(d, P, img, fx=c["fx"], cx=c["cx"])


def cast(ctx, name):
    """(maps (8, rows, cols), (n_hits, n_no_normal)) of the view on the volume the context holds"""
    _, P, v = rc.view(name)
    counts = ctx.tsdf_raycast(P, **v)
    m = ctx.tsdf_get_raycast()
    return np.concatenate([m["points"], m["normals"], m["depth"][None], m["intensity"][None]]), counts


@pytest.mark.parametrize("name", rc.TABLE + ("room_color",))
def test_maps_and_counts_match_the_model(ctx, name):
    want = rc.model(name)
    fuse(ctx, rc.view(name)[0])
    maps, counts = cast(ctx, name)
    assert counts == (want["n_hits"], want["n_no_normal"])
    if rc.VIEWS[name][3] is not None:
        assert counts == (rc.VIEWS[name][4], rc.VIEWS[name][3] - rc.VIEWS[name][4])
    for k, plane in enumerate(("x", "y", "z", "nx", "ny", "nz", "depth", "intensity")):
        assert same_bits(maps[k], want["maps"][k]), plane
    if name == "room_color":
        assert maps[7].max() > 0.1
    # the same bits from a second call, after a reset and re-integration, and on a second context
    again, counts2 = cast(ctx, name)
    assert counts2 == counts and same_bits(again, maps)
    ctx.tsdf_reset()
    with pytest.raises(binding.IcpkError) as e:  # (the maps went with the volume's contents)
        ctx.tsdf_get_raycast()
    assert e.value.code == binding.E_NOT_SET
    c = tc.case(rc.view(name)[0])
    for d, P, img in c["frames"]:
        ctx.tsdf_integrate(d, P, img, fx=c["fx"], cx=c["cx"])
    again, counts2 = cast(ctx, name)
    assert counts2 == counts and same_bits(again, maps)
    with binding.Context(0) as other:
        fuse(other, rc.view(name)[0])
        again, counts2 = cast(other, name)
        assert counts2 == counts and same_bits(again, maps)


def test_empty_volume_gives_no_hits_and_leaves_the_target(ctx):
    tgt = synth.frustum_pair(n=500, seed=3)["target"]
    ctx.set_target(tgt)
    v = tc.case("plane")["volume"]
    vol = TsdfVolume(ctx, dims=v["dims"], voxel=v["voxel"], origin=v["origin"], trunc=v["trunc"], fx=64.0, cx=31.5)
    view = {k: rc.PLANE_VIEW[k] for k in ("shape", "z_near", "z_far", "step", "min_weight")}
    r = vol.raycast(np.eye(4), **view)
    assert (r["n_hits"], r["n_no_normal"]) == (0, 0)
    assert r["points"].shape == (3, 48, 64) and not any(r[k].any() for k in ("points", "normals", "depth", "intensity"))
    with pytest.raises(binding.IcpkError) as e:
        vol.raycast_to_target(np.eye(4), **view)
    assert e.value.code == binding.E_EMPTY_TARGET
    assert same_bits(ctx.get_target(), tgt)


def pose_error(T, T_true):
    """(rotation angle in degrees, translation norm) of T T_true^-1; the angle from the skew part, which resolves small
    angles where the trace does not"""
    E = np.asarray(T, np.float64) @ np.linalg.inv(T_true)
    S = E[:3, :3] - E[:3, :3].T
    ang = np.degrees(np.arcsin(min(1.0, 0.5 * np.linalg.norm([S[2, 1], S[0, 2], S[1, 0]]))))
    return float(ang), float(np.linalg.norm(E[:3, 3]))


def test_raycast_becomes_the_target(ctx):
    c = tc.case("room_color")
    want = rc.model("room_color")["maps"]
    _, P, view = rc.view("room_color")
    vol = TsdfVolume(ctx, **{k: c["volume"][k] for k in ("dims", "voxel", "origin", "trunc")}, color=True, fx=c["fx"], cx=c["cx"])
    vol.integrate_all([f[0] for f in c["frames"]], np.stack([f[1] for f in c["frames"]]), [f[2] for f in c["frames"]])
    kw = {k: view[k] for k in ("shape", "z_near", "z_far", "step", "min_weight")}
    valid = want[6] > 0  # (boolean indexing lists the valid pixels in row-major order)
    assert vol.raycast_to_target(P, **kw) == int(valid.sum()) > 10000
    points, normals = np.ascontiguousarray(want[0:3][:, valid]), np.ascontiguousarray(want[3:6][:, valid])
    assert same_bits(ctx.get_target(), points)
    assert same_bits(ctx.get_target_normals(), normals)
    assert same_bits(ctx.get_target_colors(), np.ascontiguousarray(want[7][valid]))
    # the maps are still there, and a second hand-over gives the same target
    assert same_bits(ctx.tsdf_get_raycast()["depth"], want[6])
    ctx.tsdf_raycast_to_target()
    assert same_bits(ctx.get_target(), points)
    # the fourth frame, placed by the third frame's pose, aligned point-to-plane against the view ...
    d4, P4 = tc.room_frame(*tc.ROOM_FOURTH)
    P3 = c["frames"][2][1]
    cloud = synth.backproject(d4, None, c["fx"], c["cx"]).astype(np.float64)
    src = (P3[:3, :3] @ cloud + P3[:3, 3:4]).astype(np.float32)
    akw = dict(solve=binding.SOLVE_POINT_TO_PLANE, max_iterations=20, max_nn_dist=0.2)
    ctx.set_source(src)
    T, st, code = ctx.align(**akw)
    assoc = ctx.get_associations()
    # ... gives what a second context gives that was handed the points through the ordinary setters
    with binding.Context(0) as other:
        other.set_target(points)
        other.set_target_normals(normals)
        other.set_source(src)
        T2, st2, code2 = other.align(**akw)
        assoc2 = other.get_associations()
    assert code == code2 and same_bits(T, T2)
    assert (st.iterations, st.status, st.final_pairs) == (st2.iterations, st2.status, st2.final_pairs)
    assert np.float32(st.final_mse).tobytes() == np.float32(st2.final_mse).tobytes()
    assert np.array_equal(assoc[0], assoc2[0]) and same_bits(assoc[1], assoc2[1])
    assert code >= 0 and st.final_pairs > 5000
    err = pose_error(T, P4 @ np.linalg.inv(P3))
    print(f"fourth frame against the ray cast at its own pose: pose error {err[0]:.4f} deg, {err[1]:.5f} m")


def test_raycast_leaves_the_context_alone(ctx):
    p = synth.frustum_pair(n=3000, seed=5)
    ctx.set_target(p["target"])
    ctx.set_source(p["source"])
    ctx.map_reset()
    ctx.map_update_points(binding.MAP_ADD_CLOUD, p["target"][:, :800] + np.float32(5), 180)
    idx, dist = ctx.nn()
    fuse(ctx, "room")
    ctx.tsdf_extract_surface(1)

    def held():
        s = ctx.tsdf_get_surface()
        return (ctx.get_source(), ctx.get_target(), ctx.map_get_list(binding.MAP_POINTS), ctx.map_get_list(binding.MAP_KEYPOINTS),
                *ctx.tsdf_get()[:2], *(s[k] for k in ("points", "normals", "intensity", "voxel", "axis")))

    before = held()
    maps, counts = cast(ctx, "room")
    ctx.tsdf_raycast(rc.view("room")[1], count=False, **rc.view("room")[2])  # (and the call that does not wait)
    after = held()
    assert all(same_bits(a, b) for a, b in zip(before, after)) and before[2].shape[1] + before[3].shape[1] > 0
    assert before[6].shape[1] > 1000 and counts[0] > 10000
    i2, d2 = ctx.get_associations()
    assert np.array_equal(idx, i2) and same_bits(dist, d2)
    # integration after a ray cast leaves the maps alone: they are a snapshot
    d4, P4 = tc.room_frame(*tc.ROOM_FOURTH)
    ctx.tsdf_integrate(d4, P4, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
    ctx.tsdf_extract_surface(1)
    m = ctx.tsdf_get_raycast()
    assert same_bits(np.concatenate([m["points"], m["normals"], m["depth"][None], m["intensity"][None]]), maps)


@pytest.fixture(scope="module")
def big():
    """256^3 with one 480 x 640 frame (the recipe of test_gpu_tsdf.py's large volume): linear indices up to 2^24, 1200
    tiles of 16 x 16 pixels, 1200 chunks of 256.  The scene lies between 1.7 m and 3.7 m of depth (the sphere's front,
    the back wall), so the rays run from 1 m to 4 m: 76 samples of 0.04 m."""
    fx, cx = float(synth.FX), float(synth.CX)
    d, P = tc.room_frame((0.0, 2.0, 0.0), (0.03, 0.0, 0.0), shape=(480, 640), fx=fx, cx=cx)
    vol = dict(dims=(256, 256, 256), voxel=0.02, origin=(-2.56, -2.56, -1.0), trunc=0.08)
    m = tsdf_model.Volume(**vol)
    m.integrate(d, P, fx, cx)
    view = dict(shape=(480, 640), fx=fx, cx=cx, z_near=1.0, z_far=4.0, step=0.04, min_weight=1)
    return dict(volume=vol, fx=fx, cx=cx, depth=d, pose=P, view=view, want=rm.raycast(m, P, **view))


def test_one_image_sized_view(ctx, big):
    v = big["volume"]
    ctx.tsdf_create(dims=v["dims"], voxel=v["voxel"], origin=v["origin"], trunc=v["trunc"])
    ctx.tsdf_integrate(big["depth"], big["pose"], fx=big["fx"], cx=big["cx"])
    counts = ctx.tsdf_raycast(big["pose"], **big["view"])
    m = ctx.tsdf_get_raycast()
    want = big["want"]
    assert counts == (want["n_hits"], want["n_no_normal"]) and counts[0] > 250000
    got = np.concatenate([m["points"], m["normals"], m["depth"][None], m["intensity"][None]])
    for k in range(8):
        assert same_bits(got[k], want["maps"][k]), k
    ctx.tsdf_raycast_to_target()
    valid = want["maps"][6] > 0
    assert same_bits(ctx.get_target(), np.ascontiguousarray(want["maps"][0:3][:, valid]))
    ctx.tsdf_release()


def test_argument_checks(ctx):
    lib, h = ctx._lib, ctx._h
    _, P, v = rc.view("plane")
    ctx.tsdf_release()
    for call in (lambda: ctx.tsdf_raycast(P, **v), ctx.tsdf_get_raycast, ctx.tsdf_raycast_to_target):
        with pytest.raises(binding.IcpkError) as e:
            call()
        assert e.value.code == binding.E_NOT_SET
    assert lib.icpk_tsdf_get_raycast(h, *([None] * 8)) == binding.E_NOT_SET
    fuse(ctx, "plane")
    # before the first ray cast; after create, reset and release
    assert lib.icpk_tsdf_get_raycast(h, *([None] * 8)) == binding.E_NOT_SET
    assert lib.icpk_tsdf_raycast_to_target(h) == binding.E_NOT_SET
    maps, counts = cast(ctx, "plane")
    assert counts == (432, 240)
    tgt = synth.frustum_pair(n=500, seed=3)["target"]
    ctx.set_target(tgt)
    held = ctx.tsdf_get()
    bad = [dict(shape=(0, 64)), dict(shape=(48, -1)), dict(shape=(2048, 1025)), dict(fx=0.0), dict(fx=float("nan")),
           dict(cx=float("inf")), dict(z_near=float("nan")), dict(z_far=float("inf")), dict(step=float("nan")),
           dict(z_near=0.0), dict(z_near=-1.0), dict(z_far=0.25), dict(z_far=0.1), dict(step=-0.1),
           dict(step=2.75 / 4096), dict(min_weight=0), dict(min_weight=65536)]
    for kw in bad:
        with pytest.raises(binding.IcpkError) as e:
            ctx.tsdf_raycast(P, **dict(v, **kw))
        assert e.value.code == binding.E_ARG, kw
    for Pb in (np.full((4, 4), np.nan), np.where(np.eye(4) > 0, np.inf, 0.0)):
        with pytest.raises(binding.IcpkError) as e:
            ctx.tsdf_raycast(Pb, **v)
        assert e.value.code == binding.E_ARG
    r = binding.tsdf_raycast_params(**v)
    assert lib.icpk_tsdf_raycast(h, binding.C.byref(r), None, None, None) == binding.E_ARG
    assert lib.icpk_tsdf_raycast(None, binding.C.byref(r), None, None, None) == binding.E_ARG
    assert lib.icpk_tsdf_get_raycast(None, *([None] * 8)) == binding.E_ARG
    assert lib.icpk_tsdf_raycast_to_target(None) == binding.E_ARG
    # the intensity asked from a volume without colour
    plane = np.zeros((48, 64), np.float32)
    fp = plane.ctypes.data_as(binding.C.POINTER(binding.C.c_float))
    assert lib.icpk_tsdf_get_raycast(h, None, None, None, None, None, None, None, fp) == binding.E_ARG
    assert lib.icpk_tsdf_get_raycast(h, None, None, None, None, None, None, fp, None) == 0 and same_bits(plane, maps[6])
    # none of the refusals touched the maps, the target or the volume
    m = ctx.tsdf_get_raycast()
    assert same_bits(np.concatenate([m["points"], m["normals"], m["depth"][None], m["intensity"][None]]), maps)
    now = ctx.tsdf_get()
    assert same_bits(ctx.get_target(), tgt) and same_bits(now[0], held[0]) and same_bits(now[1], held[1])
    # step 0 is trunc / 2 (0.1875 here); N = 4096 is still allowed
    assert ctx.tsdf_raycast(P, **dict(v, step=0.0)) == counts
    m = ctx.tsdf_get_raycast()
    assert same_bits(np.concatenate([m["points"], m["normals"], m["depth"][None], m["intensity"][None]]), maps)
    ctx.tsdf_raycast(P, **dict(v, step=2.75 / 4095))
    # the maps go with the volume's contents: reset, create, release
    for gone in (ctx.tsdf_reset, lambda: fuse(ctx, "plane"), ctx.tsdf_release):
        ctx.tsdf_raycast(P, **v)
        assert lib.icpk_tsdf_get_raycast(h, *([None] * 8)) == 0
        gone()
        assert lib.icpk_tsdf_get_raycast(h, *([None] * 8)) == binding.E_NOT_SET
        assert lib.icpk_tsdf_raycast_to_target(h) == binding.E_NOT_SET
        with pytest.raises(binding.IcpkError) as e:
            ctx.tsdf_get_raycast()
        assert e.value.code == binding.E_NOT_SET


def test_model_tracker_over_the_room_frames(ctx):
    """Every frame is placed by its predecessor's true pose; the model is built from the tracker's own estimates.
    Pairs are kept within 0.1 m (1.6 voxels): the view is the model seen from the PREVIOUS pose, so what the new frame
    sees for the first time has no counterpart in it and must not pair with the view's border, and a point-to-plane
    step needs no wide gate, since an offset along a surface does not lengthen the distance to it.  Measured (DESIGN.md,
    K20): 0.026 deg / 4.7 mm, 0.58 deg / 8.5 mm, 0.10 deg / 6.8 mm after frames 1, 2, 3 against 0.54 deg / 1.35 mm frame
    to frame on the last pair; with pairs within 0.2 m the last frame came out at 0.73 deg / 13.7 mm."""
    c = tc.case("room")
    d4, P4 = tc.room_frame(*tc.ROOM_FOURTH)
    frames = [(d, P) for d, P, _ in c["frames"]] + [(d4, P4)]
    kw = dict(max_iterations=20, max_nn_dist=0.1)
    vol = TsdfVolume(ctx, **{k: c["volume"][k] for k in ("dims", "voxel", "origin", "trunc")}, fx=c["fx"], cx=c["cx"])
    tracker = ModelTracker(vol, pose=frames[0][1], z_near=0.25, z_far=6.0, step=0.125, **kw)
    errors = []
    for k, (d, P) in enumerate(frames):
        if k > 0:  # (placed by its predecessor's true pose: the estimate on top of it is the tracker's own)
            tracker.pose = frames[k - 1][1].copy()
        errors.append(pose_error(tracker.track(d), P))
    assert tracker.frames == 4 and vol.frames == 4 and tracker.n_hits > 10000 and errors[0][0] < 1e-9 and errors[0][1] < 1e-12
    # the yardstick: the last pair aligned frame to frame, the third frame's cloud with image normals as the target
    P3 = frames[2][1]
    with binding.Context(0) as other:
        other.backproject_with_normals(frames[2][0], fx=c["fx"], cx=c["cx"])
        other.set_source(synth.backproject(d4, None, c["fx"], c["cx"]))
        Tf, _, _ = other.align(solve=binding.SOLVE_POINT_TO_PLANE, **kw)
    frame_err = pose_error(Tf, np.linalg.inv(P3) @ P4)
    for k, e in enumerate(errors):
        print(f"frame {k}: frame-to-model pose error {e[0]:.4f} deg, {e[1]:.5f} m")
    print(f"last pair frame to frame: {frame_err[0]:.4f} deg, {frame_err[1]:.5f} m")
    assert errors[-1][0] <= frame_err[0]
    assert errors[-1][1] < c["volume"]["voxel"] / 2
    # a view that sees nothing of the model is refused before the alignment
    blind = ModelTracker(vol, pose=tc.pose((0, 180, 0), (0, 0, -3.0)), step=0.125, **kw)
    blind.frames = 1
    with pytest.raises(RuntimeError, match="fewer than min_pairs"):
        blind.track(d4)
    assert vol.frames == 4
