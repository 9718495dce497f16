"""The moving volume on the device (K23; icpk_tsdf_shift, _extract_leaving, _get_params, _get_box, TsdfVolume.follow,
ModelTracker(follow=...)) against tests/tsdf_shift_model.py on top of tests/tsdf_model.py, byte for byte unless said
otherwise."""
import numpy as np
import pytest

import tsdf_cases as tc
import tsdf_mesh_model
import tsdf_raycast_cases as rc
import tsdf_raycast_model
import tsdf_shift_cases as sc
import tsdf_shift_model as sm
from icp_slam_prototype_amd import binding, synth
from icp_slam_prototype_amd.tsdf import ModelTracker, TsdfVolume

pytestmark = pytest.mark.gpu

C = binding.C
LIST_KEYS = ("points", "normals", "intensity", "voxel", "axis")
MESH_ARRAYS = ("vertices", "normals", "intensity", "voxel_index", "edge", "triangles")


@pytest.fixture(scope="module")
def ctx():
    with binding.Context(0) as c:
        yield c


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def create(ctx, name):
    v = tc.case(name)["volume"]
    return ctx.tsdf_create(dims=v["dims"], voxel=v["voxel"], origin=v["origin"], trunc=v["trunc"],
                           flags=binding.TSDF_COLOR if v.get("color") else 0)


def fuse(ctx, name):
    c = tc.case(name)
    create(ctx, name)
    for d, P, img in c["frames"]:
        ctx.tsdf_integrate(d, P, img, fx=c["fx"], cx=c["cx"])


def refill(ctx, vol):
    """the model volume's planes on a volume that stands where it was created"""
    ctx.tsdf_reset()
    ctx.tsdf_set(vol.tsdf, vol.weight, vol.intensity)


def planes_are(ctx, vol):
    color = vol.intensity is not None
    f, w, ci = ctx.tsdf_get(intensity=color)
    p, total = binding.tsdf_get_params(ctx)
    return (same_bits(f, vol.tsdf) and same_bits(w, vol.weight) and (not color or same_bits(ci, vol.intensity))
            and same_bits(np.array(p.origin[:], np.float32), vol.origin)
            and np.array_equal(total, getattr(vol, "total", np.zeros(3, np.int64))))


def list_is(got, want):
    return all(same_bits(got[k], want[k]) for k in LIST_KEYS)


@pytest.mark.parametrize("name", sc.CASES)
def test_planes_after_a_shift(ctx, name):
    vol = tc.model(name)["volume"]
    fuse(ctx, name)
    assert planes_are(ctx, vol)
    for s in sc.all_shifts(vol.dims):
        refill(ctx, vol)
        binding.tsdf_shift(ctx, s)
        assert planes_are(ctx, sm.shifted(vol, s)), s
    # a second shift on top, and back: the slab that left is fresh, not restored; the origin is the creation origin
    refill(ctx, vol)
    binding.tsdf_shift(ctx, (2, 0, 1))
    once = sm.shifted(vol, (2, 0, 1))
    assert planes_are(ctx, once)
    binding.tsdf_shift(ctx, (-2, 0, -1))
    back = sm.shifted(once, (-2, 0, -1))
    assert planes_are(ctx, back) and same_bits(back.origin, vol.origin) and not same_bits(back.weight, vol.weight)
    # three steps there and one back: total is zero again and the origin has the creation origin's bits
    for s in ((1, 0, 0), (1, 0, 0), (1, 0, 0), (-3, 0, 0)):
        binding.tsdf_shift(ctx, s)
    p, total = binding.tsdf_get_params(ctx)
    assert not total.any() and same_bits(np.array(p.origin[:], np.float32), vol.origin)
    # the same bytes after a reset and re-integration, and on a second context
    s = (3, -2, 1)
    want = sm.shifted(vol, s)
    ctx.tsdf_reset()
    c = tc.case(name)
    for d, P, img in c["frames"]:
        ctx.tsdf_integrate(d, P, img, fx=c["fx"], cx=c["cx"])
    binding.tsdf_shift(ctx, s)
    assert planes_are(ctx, want)
    with binding.Context(0) as other:
        fuse(other, name)
        binding.tsdf_shift(other, s)
        assert planes_are(other, want)


@pytest.mark.parametrize("name", sc.CASES)
def test_leaving_list(ctx, name):
    m = tc.model(name)
    vol, old = m["volume"], m["surface"]
    fuse(ctx, name)
    assert ctx.tsdf_extract_surface(1) == (old["points"].shape[1], old["n_no_normal"])
    full = ctx.tsdf_get_surface()
    assert list_is(full, old)
    some = 0
    for s in sc.all_shifts(vol.dims):
        want = sm.leaving(vol, s, surface=old)
        assert binding.tsdf_extract_leaving(ctx, s, 1) == (want["points"].shape[1], want["n_no_normal"]), s
        assert list_is(ctx.tsdf_get_surface(), want), s
        some += want["points"].shape[1] > 0
        # the restriction leaks nowhere: a plain extraction afterwards is the list it was
        if s in sc.named_shifts(vol.dims):
            assert ctx.tsdf_extract_surface(1) == (old["points"].shape[1], old["n_no_normal"])
            assert list_is(ctx.tsdf_get_surface(), full)
    assert some > 10
    # a higher bar is another list, and the leaving list is what the hand-over takes
    s = (3, -2, 1)
    want = sm.leaving(vol, s, 2) if name != "odd" else sm.leaving(vol, s, 1)
    binding.tsdf_extract_leaving(ctx, s, 2 if name != "odd" else 1)
    assert list_is(ctx.tsdf_get_surface(), want) and want["points"].shape[1] > 0
    ctx.tsdf_surface_to_target()
    assert same_bits(ctx.get_target(), want["points"]) and same_bits(ctx.get_target_normals(), want["normals"])
    # the old list is the leaving list plus the list after the shift, on the device as on the model
    lv = sm.leaving(vol, s, surface=old)
    binding.tsdf_shift(ctx, s)
    n, _ = ctx.tsdf_extract_surface(1)
    after = ctx.tsdf_get_surface()
    assert n + lv["points"].shape[1] == old["points"].shape[1]
    assert np.array_equal(sm.map_back(after["voxel"], s, vol.dims), old["voxel"][lv["kept"]])
    assert same_bits(after["normals"], old["normals"][:, lv["kept"]])


def test_downstream_rules_read_the_new_origin(ctx):
    """integrate, ray cast and mesh after a shift: each would show a stale copy of the origin on the device"""
    c = tc.case("room")
    s = (3, -2, 1)
    want = sm.shifted(tc.model("room")["volume"], s)
    fuse(ctx, "room")
    binding.tsdf_shift(ctx, s)
    d4, P4 = tc.room_frame(*tc.ROOM_FOURTH)
    n = want.integrate(d4, P4, c["fx"], c["cx"])
    assert ctx.tsdf_integrate(d4, P4, fx=c["fx"], cx=c["cx"]) == n and n > 10000
    assert planes_are(ctx, want)
    view = rc.ROOM_VIEW
    ray = tsdf_raycast_model.raycast(want, P4, **view)
    assert ctx.tsdf_raycast(P4, **view) == (ray["n_hits"], ray["n_no_normal"]) and ray["n_hits"] > 10000
    g = ctx.tsdf_get_raycast()
    assert same_bits(np.concatenate([g["points"], g["normals"], g["depth"][None], g["intensity"][None]]), ray["maps"])
    mesh = tsdf_mesh_model.mesh(want, 1)
    assert ctx.tsdf_extract_mesh(1) == (mesh["n_vertices"], mesh["n_triangles"], mesh["n_no_normal"])
    got = ctx.tsdf_get_mesh()
    for k in MESH_ARRAYS:
        assert same_bits(got[k], mesh[k]), k
    assert mesh["n_triangles"] > 1000
    srf = want.extract(1)
    assert ctx.tsdf_extract_surface(1) == (srf["points"].shape[1], srf["n_no_normal"]) and list_is(ctx.tsdf_get_surface(), srf)


def test_get_box(ctx):
    vol = tc.model("odd")["volume"]
    fuse(ctx, "odd")
    f, w, _ = ctx.tsdf_get()
    dx, dy, dz = vol.dims
    boxes = [((0, 0, 0), (dx, dy, dz)), ((5, 3, 2), (6, 4, 3)), ((0, 7, 4), (dx, 8, 5)), ((1, 2, 3), (30, 17, 9)),
             ((32, 16, 8), (33, 17, 9)), ((3, 0, 0), (4, dy, dz)), ((0, 0, 8), (dx, dy, 9))]
    for lo, hi in boxes:
        bf, bw, _ = binding.tsdf_get_box(ctx, lo, hi)
        sl = tuple(slice(lo[a], hi[a]) for a in (2, 1, 0))
        assert same_bits(bf, f[sl]) and same_bits(bw, w[sl]), (lo, hi)
    bf, bw, bc = binding.tsdf_get_box(ctx, (2, 2, 2), (9, 9, 9), tsdf=False)
    assert bf is None and bc is None and same_bits(bw, w[2:9, 2:9, 2:9]) and w[2:9, 2:9, 2:9].any()
    for lo, hi in (((0, 0, 0), (dx + 1, dy, dz)), ((-1, 0, 0), (dx, dy, dz)), ((4, 4, 4), (4, 5, 5)), ((5, 4, 4), (4, 5, 5)),
                   ((0, 0, 0), (dx, dy, dz + 1)), ((0, dy, 0), (dx, dy + 1, dz))):
        with pytest.raises(binding.IcpkError) as e:
            binding.tsdf_get_box(ctx, lo, hi)
        assert e.value.code == binding.E_ARG, (lo, hi)
    with pytest.raises(binding.IcpkError) as e:  # (the volume keeps no intensities)
        binding.tsdf_get_box(ctx, (0, 0, 0), (2, 2, 2), intensity=True)
    assert e.value.code == binding.E_ARG
    i3 = (C.c_int32 * 3)(0, 0, 0)
    assert ctx._lib.icpk_tsdf_get_box(ctx._h, None, i3, None, None, None) == binding.E_ARG
    assert ctx._lib.icpk_tsdf_get_box(ctx._h, i3, None, None, None, None) == binding.E_ARG
    # a colour volume's three planes
    cvol = tc.model("room_color")["volume"]
    fuse(ctx, "room_color")
    bf, bw, bc = binding.tsdf_get_box(ctx, (60, 0, 10), (64, 64, 50), intensity=True)
    assert same_bits(bf, cvol.tsdf[10:50, :, 60:]) and same_bits(bw, cvol.weight[10:50, :, 60:])
    assert same_bits(bc, cvol.intensity[10:50, :, 60:]) and bc.max() > 0.1


def test_shift_leaves_the_context_alone_and_invalidates(ctx):
    lib, h = ctx._lib, ctx._h
    ctx.tsdf_release()
    i3 = (C.c_int32 * 3)(1, 0, 0)
    for call in (lambda: binding.tsdf_shift(ctx, (1, 0, 0)), lambda: binding.tsdf_extract_leaving(ctx, (1, 0, 0), 1), lambda: binding.tsdf_get_params(ctx),
                 lambda: binding.tsdf_get_box(ctx, (0, 0, 0), (1, 1, 1))):
        with pytest.raises(binding.IcpkError) as e:
            call()
        assert e.value.code == binding.E_NOT_SET
    assert lib.icpk_tsdf_shift(h, None) == binding.E_NOT_SET
    assert lib.icpk_tsdf_shift(None, i3) == binding.E_ARG and lib.icpk_tsdf_extract_leaving(None, 1, i3, None, None) == binding.E_ARG
    # what a context holds besides the volume
    p = synth.frustum_pair(n=3000, seed=5)
    ctx.set_target(p["target"])
    ctx.set_target_normals((p["target"] / np.linalg.norm(p["target"], axis=0)).astype(np.float32))
    ctx.set_source(p["source"])
    ctx.map_reset()
    ctx.map_update_points(binding.MAP_ADD_CLOUD, p["target"][:, :800] + np.float32(5), 180)
    idx, dist = ctx.nn()

    def held():
        return (ctx.get_source(), ctx.get_target(), ctx.get_target_normals(), ctx.map_get_list(binding.MAP_POINTS),
                ctx.map_get_list(binding.MAP_KEYPOINTS), *ctx.get_associations())

    before = held()
    vol = tc.model("room")["volume"]
    fuse(ctx, "room")
    view = rc.ROOM_VIEW
    P = tc.case("room")["frames"][2][1]
    # every refusal the header names leaves the planes, the origin and the lists as they were
    ctx.tsdf_extract_surface(1)
    full = ctx.tsdf_get_surface()
    assert lib.icpk_tsdf_shift(h, None) == binding.E_ARG
    assert lib.icpk_tsdf_extract_leaving(h, 1, None, None, None) == binding.E_ARG
    for mw in (0, -3, 65536):
        with pytest.raises(binding.IcpkError) as e:
            binding.tsdf_extract_leaving(ctx, (1, 0, 0), mw)
        assert e.value.code == binding.E_ARG
    assert planes_are(ctx, vol) and list_is(ctx.tsdf_get_surface(), full)
    assert lib.icpk_tsdf_get_params(h, None, None) == 0
    # s = 0 succeeds and is a no-op: the lists stay
    ctx.tsdf_raycast(P, **view)
    ctx.tsdf_extract_mesh(1)
    binding.tsdf_shift(ctx, (0, 0, 0))
    assert planes_are(ctx, vol) and list_is(ctx.tsdf_get_surface(), full)
    assert lib.icpk_tsdf_get_raycast(h, *([None] * 8)) == 0 and lib.icpk_tsdf_get_mesh(h, *([None] * 10)) == 0
    # a shift drops the surface list, the ray-cast maps and the mesh, and nothing else
    binding.tsdf_shift(ctx, (1, 0, -2))
    assert lib.icpk_tsdf_get_surface(h, *([None] * 9)) == binding.E_NOT_SET
    assert lib.icpk_tsdf_get_raycast(h, *([None] * 8)) == binding.E_NOT_SET
    assert lib.icpk_tsdf_get_mesh(h, *([None] * 10)) == binding.E_NOT_SET
    assert lib.icpk_tsdf_surface_to_target(h) == binding.E_NOT_SET and lib.icpk_tsdf_raycast_to_target(h) == binding.E_NOT_SET
    for getter in (ctx.tsdf_get_surface, ctx.tsdf_get_raycast, ctx.tsdf_get_mesh):
        with pytest.raises(binding.IcpkError) as e:
            getter()
        assert e.value.code == binding.E_NOT_SET
    after = held()
    assert all(same_bits(a, b) for a, b in zip(before, after)) and before[3].shape[1] + before[4].shape[1] > 0
    assert np.array_equal(idx, after[5]) and same_bits(dist, after[6])
    # a target handed over from this volume earlier stays when the volume moves on
    ctx.tsdf_extract_surface(1)
    ctx.tsdf_surface_to_target()
    tgt, nrm = ctx.get_target(), ctx.get_target_normals()
    binding.tsdf_shift(ctx, (-4, 2, 0))
    assert same_bits(ctx.get_target(), tgt) and same_bits(ctx.get_target_normals(), nrm) and tgt.shape[1] > 1000
    # reset puts the box back where it was created; set leaves the cumulative shift
    ctx.tsdf_set(vol.tsdf, vol.weight)
    _, total = binding.tsdf_get_params(ctx)
    assert total.tolist() == [-3, 2, -2]
    ctx.tsdf_reset()
    p, total = binding.tsdf_get_params(ctx)
    assert not total.any() and same_bits(np.array(p.origin[:], np.float32), vol.origin) and not ctx.tsdf_get()[1].any()


def test_fusion_through_a_moving_box(ctx):
    """A walk of 1.875 m along x through a box 2 m wide that follows the camera two voxels at a time: the planes, every
    streamed list and the final surface are the bytes of the same loop on the numpy models; together the lists span
    more than the box and lie on the analytic room."""
    want = sc.walk_model()
    v = sc.WALK_VOLUME
    vol = TsdfVolume(ctx, dims=v["dims"], voxel=v["voxel"], origin=v["origin"], trunc=v["trunc"], fx=tc.ROOM_FX, cx=tc.ROOM_CX)
    vol.follow_min_weight = 1
    streamed, updated = [], []
    for d, P in sc.walk_frames():
        left = vol.follow(P, every=sc.WALK_EVERY)
        if left is not None:
            streamed.append(left)
        updated.append(vol.integrate(d, P))
    assert updated == want["n_updated"] and len(streamed) == len(want["streamed"]) == 15
    assert vol.total.tolist() == [30, 0, 0] and planes_are(ctx, want["volume"])
    assert np.float32(vol.params.origin[0]) == want["volume"].origin[0] == np.float32(0.875)
    for k, (got, w) in enumerate(zip(streamed, want["streamed"])):
        assert list_is(got, w), k
    final = vol.surface(1)
    assert list_is(final, want["final"]) and vol.n_no_normal == want["final"]["n_no_normal"]
    # the two conditions the walk was chosen for (they hold on the numpy loop; here on the device's lists)
    union = sc.walk_union(streamed, final)
    width = v["dims"][0] * v["voxel"]
    assert union[0].max() - union[0].min() > width == 2.0
    near = tc.room_distance(union) <= v["voxel"] / 2
    print(f"{union.shape[1]} points over {union[0].max() - union[0].min():.3f} m in x, {near.mean():.4f} within half a voxel of the room")
    assert near.mean() >= 0.99 and union.shape[1] > 2000
    # the box wraps the slab it is about to lose, losslessly
    bf, bw, _ = vol.box((0, 0, 0), (2, 64, 64))
    f, w, _ = vol.planes()
    assert same_bits(bf, f[:, :, :2]) and same_bits(bw, w[:, :, :2]) and bw.any()


def pose_error(T, T_true):
    """(rotation angle in degrees, translation norm) of T T_true^-1 (tests/test_gpu_tsdf_raycast.py's)"""
    E = np.asarray(T, np.float64) @ np.linalg.inv(T_true)
    S = E[:3, :3] - E[:3, :3].T
    ang = np.degrees(np.arcsin(min(1.0, 0.5 * np.linalg.norm([S[2, 1], S[0, 2], S[1, 0]]))))
    return float(ang), float(np.linalg.norm(E[:3, 3]))


def run_tracker(ctx, follow):
    """test_model_tracker_over_the_room_frames's set-up (tests/test_gpu_tsdf_raycast.py)"""
    c = tc.case("room")
    d4, P4 = tc.room_frame(*tc.ROOM_FOURTH)
    frames = [(d, P) for d, P, _ in c["frames"]] + [(d4, P4)]
    kw = dict(max_iterations=20, max_nn_dist=0.1)
    vol = TsdfVolume(ctx, **{k: c["volume"][k] for k in ("dims", "voxel", "origin", "trunc")}, fx=c["fx"], cx=c["cx"])
    tracker = ModelTracker(vol, pose=frames[0][1], z_near=0.25, z_far=6.0, step=0.125, follow=follow, **kw)
    poses, totals, streamed = [], [], []
    for k, (d, P) in enumerate(frames):
        if k > 0:
            tracker.pose = frames[k - 1][1].copy()
        poses.append(tracker.track(d))
        totals.append(vol.total.copy())
        streamed.append(sum(s["points"].shape[1] for s in tracker.streamed))
    return tracker, vol, frames, poses, totals, streamed, kw


def test_tracker_follows_and_equals_where_nothing_is_lost(ctx):
    """ModelTracker(follow=1) against ModelTracker(follow=None) over the room frames.  Frame 1 moves the camera 0.96
    voxel in x: once its pose is found the volume shifts by (1, 0, 0), which on `room` loses no crossing (nothing is
    streamed), so the pose of frame 2 is found against the same model but for the rounding of the new origin -- in the
    ray cast, and in the voxel centres frame 1 is fused at.  The poses of frames 0 and 1 are found before any shift.
    The walk does not end with that one shift, though: frame 2 stands 1.8 voxels behind the new reference in x (and
    half a voxel off in y), so the volume then shifts by (-2, 1, 0), which streams 166 crossings and drops voxels the
    next view would have seen; the pose of frame 3 is therefore held to the tracker's own bars and not to the
    agreement.  Measured on the device (following against fixed volume): frame 1 4e-16 deg / 7e-18 m, frame 2 0.00135
    deg / 6.6e-5 m, frame 3 0.0051 deg / 1.3e-4 m.  Ten times the frame-2 figures is looser than 0.01 deg / 1e-4 m, so
    these two are the bounds.  The following tracker's own errors: 0.026 deg / 4.7 mm, 0.58 deg / 8.4 mm, 0.106 deg /
    6.8 mm against 0.54 deg / 1.35 mm frame to frame on the last pair."""
    plain = run_tracker(ctx, None)
    tracker, vol, frames, poses, totals, streamed, kw = run_tracker(ctx, 1)
    assert plain[0].shifts == 0 and not plain[1].total.any() and plain[0].streamed == []
    # the shift happened where the arithmetic says, by (1, 0, 0), and streamed nothing
    diffs = [pose_error(a, b) for a, b in zip(poses, plain[3])]
    for k, e in enumerate(diffs):
        print(f"frame {k}: following vs fixed volume {e[0]:.3g} deg, {e[1]:.3g} m; shift so far {totals[k].tolist()}, "
              f"streamed so far {streamed[k]}")
    assert [t.tolist() for t in totals[:2]] == [[0, 0, 0], [1, 0, 0]] and streamed[1] == 0 and tracker.shifts >= 1
    # the tracker's own bars hold on the following tracker, against the same yardstick
    errors = [pose_error(T, P) for T, (_, P) in zip(poses, frames)]
    c = tc.case("room")
    P3, (d4, P4) = frames[2][1], frames[3]
    with binding.Context(0) as other:
        other.backproject_with_normals(frames[2][0], fx=c["fx"], cx=c["cx"])
        other.set_source(synth.backproject(d4, None, c["fx"], c["cx"]))
        Tf, _, _ = other.align(solve=binding.SOLVE_POINT_TO_PLANE, **kw)
    frame_err = pose_error(Tf, np.linalg.inv(P3) @ P4)
    for k, e in enumerate(errors):
        print(f"frame {k}: following tracker's pose error {e[0]:.4f} deg, {e[1]:.5f} m")
    print(f"last pair frame to frame: {frame_err[0]:.4f} deg, {frame_err[1]:.5f} m")
    assert tracker.frames == 4 and vol.frames == 4
    # measured 0 deg / 0 m on frames 0 .. 2: ten times that is below the floor the bound may not
    # go under, so the floor it is
    for e in diffs[:3]:  # (the poses found before any shift and after the lossless one)
        assert e[0] <= 0.01 and e[1] <= 1e-4
    assert streamed[2] > 0  # (the second shift is not lossless: what it streams is what the fixed volume still holds)
    assert errors[-1][0] <= frame_err[0]
    assert errors[-1][1] < c["volume"]["voxel"] / 2
