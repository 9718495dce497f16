"""K22 on the device: icpk_bilateral_depth_image against tests/bilateral_model.py, byte for byte (every case feeds the
library's tables to the model); icpk_backproject_smoothed against the two-call sequence through the host; what the calls
leave alone; a reused context against fresh ones; tsdf.ModelTracker(bilateral=True) against the hand-written loop; and
every refusal the header names."""
import ctypes as C

import numpy as np
import pytest

import bilateral_model as bm
import tsdf_cases as tc
from icp_slam_prototype_amd import binding, depth, synth
from icp_slam_prototype_amd.tsdf import ModelTracker, TsdfVolume

pytestmark = pytest.mark.gpu

U16 = C.POINTER(C.c_uint16)


@pytest.fixture(scope="module")
def ctx():
    with binding.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def big():
    """(image, params, the model's bytes) of the one 480 x 640 frame: computed once, read-only"""
    img, fields = bm.case("room_480x640")
    p = depth.bilateral_params(**fields)
    want = bm.bilateral(img, *depth.bilateral_tables(p))
    want.setflags(write=False)
    return img, p, want


def expect(name):
    img, fields = bm.case(name)
    p = depth.bilateral_params(**fields)
    return img, p, bm.bilateral(img, *depth.bilateral_tables(p))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def code_of(call, *a, **kw):
    with pytest.raises(binding.IcpkError) as e:
        call(*a, **kw)
    return e.value.code


@pytest.mark.parametrize("name", bm.HOST_CASES + bm.TILE_CASES)
def test_device_gives_the_models_bytes(ctx, name):
    img, p, want = expect(name)
    got = depth.bilateral_depth_image(ctx, img, p)
    assert same_bits(got, want)
    assert same_bits(got, depth.bilateral_host(img, p))
    if name in bm.UNCHANGED:
        assert same_bits(got, np.array(img))


@pytest.mark.parametrize("radius", [1, 3, 6])
def test_every_radius_on_a_frame_of_several_tiles(ctx, radius):
    img, _ = bm.case("33x129")
    p = depth.bilateral_params(radius=radius, sigma_space=radius / 1.5)
    assert same_bits(depth.bilateral_depth_image(ctx, img, p), bm.bilateral(img, *depth.bilateral_tables(p)))
    wide = depth.bilateral_params(radius=radius, sigma_range=700.0)  # K = 2101: most of the range table is staged
    noisy = (np.array(img, np.int64) * 3 % 2000 + 1000).astype(np.uint16) * (np.array(img) != 0)
    assert same_bits(depth.bilateral_depth_image(ctx, noisy, wide), bm.bilateral(noisy, *depth.bilateral_tables(wide)))


def test_full_frame_second_call_in_place_and_second_context(ctx, big):
    img, p, want = big
    assert same_bits(depth.bilateral_depth_image(ctx, img, p), want)
    assert same_bits(depth.bilateral_depth_image(ctx, img, p), want)  # a second call
    buf = np.array(img)
    assert depth.bilateral_depth_image(ctx, buf, p, out=buf) is buf and same_bits(buf, want)  # depth_out is depth_in
    assert same_bits(depth.bilateral_depth_image(ctx, img, None), want)  # NULL: the defaults
    with binding.Context(0) as other:
        assert same_bits(depth.bilateral_depth_image(other, img, p), want)


@pytest.mark.parametrize("which", [0, 1])
def test_backproject_smoothed_equals_the_two_calls(ctx, which):
    img, p, want = expect("room_masked")
    fx, cx = bm.intrinsics(120)
    off = np.float32([5, 5, 5])
    get = ctx.get_source if which == 0 else ctx.get_target
    n = depth.backproject_smoothed(ctx, img, which=which, fx=fx, cx=cx, offset=off, params=p)
    got = get()
    with binding.Context(0) as ref:
        m = ref.backproject(depth.bilateral_depth_image(ref, img, p), which=which, fx=fx, cx=cx, offset=off)
        ref_pts = ref.get_source() if which == 0 else ref.get_target()
    assert n == m == int((img != 0).sum()) and same_bits(got, ref_pts)
    assert same_bits(got, synth.backproject(want, None, fx, cx) + off[:, None])


@pytest.mark.parametrize("mode", [binding.NORMALS_CROSS, binding.NORMALS_REFERENCE])
def test_backproject_smoothed_with_normals(ctx, mode):
    img, p, _ = expect("room_120x160")
    fx, cx = bm.intrinsics(120)
    n = depth.backproject_smoothed(ctx, img, which=1, normals_mode=mode, fx=fx, cx=cx, params=p)
    pts, nrm = ctx.get_target(), ctx.get_target_normals()
    with binding.Context(0) as ref:
        m = ref.backproject_with_normals(depth.bilateral_depth_image(ref, img, p), mode, fx=fx, cx=cx)
        assert n == m and same_bits(pts, ref.get_target()) and same_bits(nrm, ref.get_target_normals())
    assert n == int((img != 0).sum()) and np.any(nrm != 0)


def test_what_the_calls_leave_alone():
    img, p, _ = expect("room_masked")
    other, _ = bm.case("room_120x160")
    fx, cx = bm.intrinsics(120)
    c = tc.case("room")
    with binding.Context(0) as ctx:
        ctx.backproject(other, which=1, fx=fx, cx=cx)
        ctx.backproject(img, which=0, fx=fx, cx=cx)
        ctx.nn()
        ctx.tsdf_create(**{k: c["volume"][k] for k in ("dims", "voxel", "origin", "trunc")})
        ctx.tsdf_integrate(c["frames"][0][0], c["frames"][0][1], fx=c["fx"], cx=c["cx"])
        ctx.map_reset()
        ctx.map_update_points(binding.MAP_ADD_CLOUD, ctx.get_target()[:, ::7] + np.float32(5), 180)  # the key-point list
        ctx.map_set_points(binding.MAP_FROM_TARGET)  # ... and the point list

        def state():
            s = [ctx.get_source(), *ctx.tsdf_get()[:2], ctx.map_get_list(binding.MAP_KEYPOINTS), ctx.map_get_list(binding.MAP_POINTS)]
            return b"".join(np.ascontiguousarray(a).tobytes() for a in s)

        def clouds():
            return b"".join(a.tobytes() for a in (ctx.get_target(), *ctx.get_associations()))

        before, before_clouds = state(), clouds()
        assert ctx.map_size(binding.MAP_KEYPOINTS) > 100 and ctx.map_size(binding.MAP_POINTS) == ctx.target_size
        # the filter alone touches no cloud: everything, the target and the associations included, stays
        depth.bilateral_depth_image(ctx, img, p)
        assert state() == before and clouds() == before_clouds
        # a smoothed target: the source, the volume and the map stay; the associations go with the target they were
        # made against, exactly as after backproject / backproject_filtered
        depth.backproject_smoothed(ctx, img, which=1, fx=fx, cx=cx, params=p)
        assert state() == before and ctx.get_target().tobytes() != before_clouds[:12 * ctx.target_size]
        assert code_of(ctx.get_associations) == binding.E_NOT_SET
        with binding.Context(0) as ref:
            ref.backproject(other, which=1, fx=fx, cx=cx)
            ref.backproject(img, which=0, fx=fx, cx=cx)
            ref.nn()
            ref.backproject_filtered(img, which=1, fx=fx, cx=cx)
            assert code_of(ref.get_associations) == binding.E_NOT_SET
        # the image buffers are shared with backproject_pair's resident frame: none is resident afterwards
        for call in (lambda: depth.backproject_smoothed(ctx, img, which=1, fx=fx, cx=cx, params=p),
                     lambda: depth.bilateral_depth_image(ctx, img, p),
                     lambda: ctx.backproject_filtered(img, which=1, fx=fx, cx=cx)):
            ctx.backproject_pair(img, other, fx=fx, cx=cx)
            ctx.backproject_pair(other, None, fx=fx, cx=cx)  # (resident: accepted)
            call()
            assert code_of(ctx.backproject_pair, img, None, fx=fx, cx=cx) == binding.E_NOT_SET


def test_a_reused_context_gives_fresh_contexts_bytes(ctx, big):
    """The image buffers are shared by K4, K6 and K22, and the tables stay on the device between calls: one context
    filters the large frame, then a small one with other parameters, then runs K6 + back-projection + NN on the small
    frame, and gives at every step what a context that has done nothing else gives."""
    img, p, want = big
    small, fields = bm.case("room_37x53")
    small2 = np.array(bm.case("room_120x160")[0][41:78, 61:114])
    q = depth.bilateral_params(**dict(fields, radius=2, sigma_range=11.0))
    fx, cx = bm.intrinsics(120)

    def front(c):
        flt = c.filter_depth_image(small, max_d=20000, min_d=1000)
        n = (c.backproject(flt, which=1, fx=fx, cx=cx), c.backproject(small2, which=0, fx=fx, cx=cx))
        idx, dist = c.nn()
        return flt.tobytes() + c.get_target().tobytes() + c.get_source().tobytes() + idx.tobytes() + dist.tobytes(), n

    with binding.Context(0) as used:
        assert same_bits(depth.bilateral_depth_image(used, img, p), want)
        got_small = depth.bilateral_depth_image(used, small, q)
        got_front = front(used)
        again = depth.bilateral_depth_image(used, small, q)
    with binding.Context(0) as fresh:
        assert same_bits(got_small, depth.bilateral_depth_image(fresh, small, q))
    assert same_bits(got_small, bm.bilateral(small, *depth.bilateral_tables(q))) and same_bits(again, got_small)
    with binding.Context(0) as fresh:
        assert got_front == front(fresh) and min(got_front[1]) > 1000


def noisy_room_frames():
    """the three frames of the TSDF room case with sensor noise: (depth, true pose)"""
    rng = np.random.default_rng(5)
    out = []
    for rot, shift in tc.ROOM_MOTIONS:
        P = tc.pose(rot, shift)
        out.append((synth.render_room_depth(*tc.ROOM_SHAPE, P[:3, :3], P[:3, 3], tc.ROOM_FX, tc.ROOM_CX, 0.002, rng), P))
    return out


def test_model_tracker_with_smoothing_is_the_hand_written_loop(ctx):
    frames = noisy_room_frames()
    kw = dict(max_iterations=12, max_nn_dist=0.1)
    geom = {k: tc.ROOM_VOLUME[k] for k in ("dims", "voxel", "origin", "trunc")}
    p = depth.bilateral_params()
    vol = TsdfVolume(ctx, **geom, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
    tracker = ModelTracker(vol, pose=frames[0][1], step=0.125, bilateral=True, **kw)
    poses = [tracker.track(d) for d, _ in frames]
    planes = vol.planes()
    assert tracker.bilateral.radius == 3 and tracker.frames == 3
    with binding.Context(0) as hand:
        hand.tsdf_create(**geom)
        pose, by_hand = frames[0][1].copy(), []
        for k, (d, _) in enumerate(frames):
            if k > 0:
                hand.tsdf_raycast(pose, shape=d.shape, fx=tc.ROOM_FX, cx=tc.ROOM_CX, z_near=0.25, z_far=6.0, step=0.125, min_weight=1)
                hand.tsdf_raycast_to_target()
                depth.backproject_smoothed(hand, d, which=0, fx=tc.ROOM_FX, cx=tc.ROOM_CX, params=p)
                hand.transform_source(pose[:3, :3], pose[:3, 3])
                hand.commit_source()
                T, _, _ = hand.align(solve=binding.SOLVE_POINT_TO_PLANE, **kw)
                pose = T.astype(np.float64) @ pose
            hand.tsdf_integrate(d, pose, fx=tc.ROOM_FX, cx=tc.ROOM_CX)  # the RAW frame
            by_hand.append(pose.copy())
    assert all(same_bits(a, b) for a, b in zip(poses, by_hand))
    assert not np.array_equal(poses[1], frames[0][1]) and not np.array_equal(poses[2], poses[1])
    # the volume holds the raw frames at those poses, not the smoothed ones
    with binding.Context(0) as raw:
        raw.tsdf_create(**geom)
        for (d, _), P in zip(frames, poses):
            raw.tsdf_integrate(d, P, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
        want = raw.tsdf_get()
        raw.tsdf_reset()
        for (d, _), P in zip(frames, poses):
            raw.tsdf_integrate(depth.bilateral_host(d, p), P, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
        smoothed = raw.tsdf_get()
    assert same_bits(planes[0], want[0]) and same_bits(planes[1], want[1])
    assert not same_bits(planes[0], smoothed[0])  # (the comparison can tell the two apart)
    # bilateral=None is the path without the filter
    vol2 = TsdfVolume(ctx, **geom, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
    plain = ModelTracker(vol2, pose=frames[0][1], step=0.125, **kw)
    plain_poses = [plain.track(d) for d, _ in frames]
    assert plain.bilateral is None and not same_bits(plain_poses[2], poses[2])


def pose_error(T, truth):
    E = np.linalg.inv(truth) @ np.asarray(T, np.float64)
    return float(np.degrees(np.arccos(np.clip((np.trace(E[:3, :3]) - 1) / 2, -1, 1)))), float(np.linalg.norm(E[:3, 3]))


def test_pose_error_of_a_noisy_pair_is_reported(ctx):
    """Point-to-plane alignment of the second noisy room frame onto the first (image normals on the target), with the raw
    frames and with both smoothed.  Printed for DESIGN.md (K22); nothing is asserted about the error, because nobody
    has measured it before."""
    (d0, P0), (d1, P1) = noisy_room_frames()[:2]
    truth = np.linalg.inv(P0) @ P1
    kw = dict(solve=binding.SOLVE_POINT_TO_PLANE, max_iterations=20, max_nn_dist=0.1)
    ctx.backproject_with_normals(d0, binding.NORMALS_CROSS, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
    ctx.backproject(d1, which=0, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
    raw = pose_error(ctx.align(**kw)[0], truth)
    depth.backproject_smoothed(ctx, d0, which=1, normals_mode=binding.NORMALS_CROSS, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
    depth.backproject_smoothed(ctx, d1, which=0, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
    smooth = pose_error(ctx.align(**kw)[0], truth)
    print(f"noisy pair, point to plane: raw {raw[0]:.4f} deg {raw[1] * 1000:.2f} mm; smoothed {smooth[0]:.4f} deg "
          f"{smooth[1] * 1000:.2f} mm")
    assert all(np.isfinite(v) for v in raw + smooth)


def test_every_refusal(ctx):
    img, p, _ = expect("room_37x53")
    lib, h = ctx._lib, ctx._h
    a = np.array(img)
    out = np.full(img.shape, 7, np.uint16)
    ap, op = a.ctypes.data_as(U16), out.ctypes.data_as(U16)
    rows, cols = img.shape
    ctx.backproject(a, which=0)
    ctx.backproject(a, which=1)
    src, tgt = ctx.get_source(), ctx.get_target()
    bad = [depth.bilateral_params(**f) for f in (dict(radius=0), dict(radius=7), dict(sigma_space=0.0),
                                                 dict(sigma_space=float("nan")), dict(sigma_range=-1.0),
                                                 dict(sigma_range=float("inf")), dict(range_cutoff=-1),
                                                 dict(range_cutoff=4097), dict(sigma_range=1365.4))]
    E = binding.E_ARG
    for q in bad:
        assert lib.icpk_bilateral_depth_image(h, C.byref(q), ap, op, rows, cols) == E
        assert lib.icpk_backproject_smoothed(h, ap, rows, cols, 468.6, 318.27, None, 0, -1, C.byref(q)) == E
        assert code_of(depth.bilateral_depth_image, ctx, a, q) == E
    P = C.byref(p)
    assert lib.icpk_bilateral_depth_image(None, P, ap, op, rows, cols) == E
    assert lib.icpk_bilateral_depth_image(h, P, None, op, rows, cols) == E
    assert lib.icpk_bilateral_depth_image(h, P, ap, None, rows, cols) == E
    for r, c in ((0, cols), (rows, 0), (-1, cols), (1 << 14, (1 << 14) + 1)):
        assert lib.icpk_bilateral_depth_image(h, P, ap, op, r, c) == E
        assert lib.icpk_backproject_smoothed(h, ap, r, c, 468.6, 318.27, None, 0, -1, P) == E
    assert lib.icpk_backproject_smoothed(None, ap, rows, cols, 468.6, 318.27, None, 0, -1, P) == E
    assert lib.icpk_backproject_smoothed(h, None, rows, cols, 468.6, 318.27, None, 0, -1, P) == E
    for which in (-1, 2):
        assert lib.icpk_backproject_smoothed(h, ap, rows, cols, 468.6, 318.27, None, which, -1, P) == E
    assert lib.icpk_backproject_smoothed(h, ap, rows, cols, 468.6, 318.27, None, 0, binding.NORMALS_CROSS, P) == E
    assert lib.icpk_backproject_smoothed(h, ap, rows, cols, 468.6, 318.27, None, 1, binding.NORMALS_REFERENCE + 1, P) == E
    assert code_of(depth.backproject_smoothed, ctx, a, which=0, normals_mode=binding.NORMALS_CROSS) == E
    # a refused call leaves everything as it was
    assert np.all(out == 7) and same_bits(ctx.get_source(), src) and same_bits(ctx.get_target(), tgt)
    with pytest.raises(ValueError):
        depth.bilateral_depth_image(ctx, a, p, out=np.zeros((3, 3), np.uint16))
