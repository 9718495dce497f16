"""K24 on the device: icpk_depth_pyramid_build against tests/pyramid_model.py and the host function, byte for byte, for
every case and level count; with smoothing against the model over depth.bilateral_host; a second build, a reused and a
second context; backproject_level against Context.backproject / backproject_with_normals of the downloaded level; what
build leaves alone; every refusal; tsdf.ModelTracker(pyramid=...) against the loop written out by hand; and what the
pyramid buys on the room scene, measured."""
import ctypes as C

import numpy as np
import pytest

import bilateral_model as bm
import pyramid_model as pm
import tsdf_cases as tc
from icp_slam_prototype_amd import binding, depth, synth
from icp_slam_prototype_amd.tsdf import ModelTracker, TsdfVolume

pytestmark = pytest.mark.gpu

U16 = C.POINTER(C.c_uint16)
FP = C.POINTER(C.c_float)
GEOM = {k: tc.ROOM_VOLUME[k] for k in ("dims", "voxel", "origin", "trunc")}


@pytest.fixture(scope="module")
def ctx():
    with binding.Context(0) as c:
        yield c


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def code_of(call, *a, **kw):
    with pytest.raises(binding.IcpkError) as e:
        call(*a, **kw)
    return e.value.code


def levels_of(c, n):
    return [depth.pyramid_level(c, l) for l in range(n)]


@pytest.mark.parametrize("name", pm.HOST_CASES + pm.TILE_CASES)
def test_device_gives_the_models_bytes(ctx, name):
    img, K = pm.case(name)
    want = pm.expected(name)
    for levels in pm.LEVEL_COUNTS:
        p = depth.pyramid_params(levels=levels, range_cutoff=K)
        assert depth.build_pyramid(ctx, img, p) == pm.shapes(img.shape, levels)
        got = levels_of(ctx, levels)
        for l in range(levels):
            assert depth.pyramid_shape(ctx, l) == want[l].shape
            assert same_bits(got[l], np.array(want[l])), (levels, l)
            assert same_bits(got[l], depth.pyramid_host(img, l, p)), (levels, l)
            if l and name in pm.SUBSAMPLED:
                assert same_bits(got[l], np.ascontiguousarray(got[l - 1][::2, ::2]))
        assert code_of(depth.pyramid_level, ctx, levels) == binding.E_ARG  # the pyramid ends there
    if name == "room_37x53":
        assert got[-1].shape == (1, 1) and got[-2].shape == (1, 1)  # 1 x 1 stays 1 x 1


def test_full_frame_defaults_smoothing_and_a_second_context(ctx):
    """the one 480 x 640 frame: the defaults are one launch of both stages over 40 x 30 workgroups"""
    img, K = pm.case("room_480x640")
    want = pm.expected("room_480x640")
    assert K == pm.DEFAULT_K and depth.build_pyramid(ctx, img) == [(480, 640), (240, 320), (120, 160)]  # NULL: the defaults
    assert all(same_bits(a, np.array(b)) for a, b in zip(levels_of(ctx, 3), want))
    b = depth.bilateral_params()
    smooth = pm.pyramid(depth.bilateral_host(img, b), 3, K)
    assert not same_bits(smooth[2], np.array(want[2]))
    depth.build_pyramid(ctx, img, None, smooth=b)
    assert all(same_bits(a, s) for a, s in zip(levels_of(ctx, 3), smooth))
    with binding.Context(0) as other:
        depth.build_pyramid(other, img, depth.pyramid_params())
        assert all(same_bits(a, np.array(w)) for a, w in zip(levels_of(other, 3), want))


@pytest.mark.parametrize("name", ["room_masked", "17x65"])
def test_with_smoothing_level_0_is_the_filtered_frame(ctx, name):
    img, K = pm.case(name)
    b = depth.bilateral_params(radius=2, sigma_range=20.0)
    p = depth.pyramid_params(levels=4, range_cutoff=K)
    want = pm.pyramid(depth.bilateral_host(img, b), 4, K)
    depth.build_pyramid(ctx, img, p, smooth=b)
    assert all(same_bits(a, w) for a, w in zip(levels_of(ctx, 4), want))
    assert not same_bits(want[0], np.array(img))


def test_a_second_build_replaces_the_first_and_a_reused_context_is_a_fresh_one():
    big, Kb = pm.case("68x260")
    small, Ks = pm.case("room_37x53")
    with binding.Context(0) as used:
        depth.build_pyramid(used, big, depth.pyramid_params(levels=8, range_cutoff=Kb))
        assert depth.pyramid_shape(used, 7) == (1, 3)
        depth.build_pyramid(used, small, depth.pyramid_params(levels=2, range_cutoff=Ks))  # another shape, fewer levels
        got = levels_of(used, 2)
        assert code_of(depth.pyramid_level, used, 2) == binding.E_ARG and code_of(depth.pyramid_shape, used, 2) == binding.E_ARG
        depth.build_pyramid(used, big, depth.pyramid_params(levels=3, range_cutoff=Kb), smooth=depth.bilateral_params())
        depth.build_pyramid(used, small, depth.pyramid_params(levels=2, range_cutoff=Ks))
        again = levels_of(used, 2)
    with binding.Context(0) as fresh:
        depth.build_pyramid(fresh, small, depth.pyramid_params(levels=2, range_cutoff=Ks))
        first = levels_of(fresh, 2)
    want = pm.expected("room_37x53")
    for l in range(2):
        assert same_bits(got[l], first[l]) and same_bits(again[l], first[l]) and same_bits(first[l], np.array(want[l]))


CLOUD_CASES = [(0, None), (1, None), (1, binding.NORMALS_CROSS), (1, binding.NORMALS_REFERENCE)]


@pytest.mark.parametrize("which,mode", CLOUD_CASES)
def test_backproject_level_is_backproject_of_the_level(which, mode):
    """on fresh contexts: the points, the normals and the counts are the same bits, with the subsampling off and on
    (the second pair of calls draws the second key on both sides)"""
    img, K = pm.case("room_120x160")
    fx, cx = bm.intrinsics(120)
    off = np.float32([5, 5, 5])
    p = depth.pyramid_params(levels=3, range_cutoff=K)
    with binding.Context(0) as a, binding.Context(0) as b:
        depth.build_pyramid(a, img, p)
        for factor in (0, 3):
            a.set_subsample(factor, 11)
            b.set_subsample(factor, 11)
            for l in (2, 0, 1):
                lvl = depth.pyramid_level(a, l)
                n = depth.backproject_level(a, l, which=which, normals_mode=mode, fx=fx, cx=cx, offset=off)
                if mode is None:
                    m = b.backproject(lvl, which=which, fx=fx / 2 ** l, cx=cx / 2 ** l, offset=off)
                else:
                    m = b.backproject_with_normals(lvl, mode, fx=fx / 2 ** l, cx=cx / 2 ** l, offset=off)
                assert n == m and (n == int((lvl != 0).sum()) if factor == 0 else 0 < n < int((lvl != 0).sum()))
                pa, pb = (c.get_source() if which == 0 else c.get_target() for c in (a, b))
                assert same_bits(pa, pb)
                if factor == 0 and mode is None:
                    assert same_bits(pa, synth.backproject(lvl, None, fx / 2 ** l, cx / 2 ** l) + off[:, None])
                if mode is not None:
                    na, nb = a.get_target_normals(), b.get_target_normals()
                    assert same_bits(na, nb) and np.any(na != 0)
                else:
                    assert (a.source_size, a.target_size) == (b.source_size, b.target_size)


def test_what_build_leaves_alone_and_what_backproject_level_drops():
    img, K = pm.case("room_masked")
    other, _ = pm.case("room_120x160")
    fx, cx = bm.intrinsics(120)
    with binding.Context(0) as ctx:
        ctx.backproject_pair(img, other, fx=fx, cx=cx)  # `img` is the resident frame now
        ctx.nn()

        def state():
            return b"".join(a.tobytes() for a in (ctx.get_source(), ctx.get_target(), *ctx.get_associations()))

        before = state()
        depth.build_pyramid(ctx, other, depth.pyramid_params(levels=4, range_cutoff=K))
        assert state() == before  # clouds and associations
        assert ctx.backproject_pair(other, None, fx=fx, cx=cx)[0] > 1000  # (resident: accepted) -- the frame stayed
        ctx.nn()
        before = state()
        # with smoothing the upload goes through the shared image buffers: the clouds stay, the resident frame goes
        depth.build_pyramid(ctx, other, None, smooth=depth.bilateral_params())
        assert state() == before
        assert code_of(ctx.backproject_pair, img, None, fx=fx, cx=cx) == binding.E_NOT_SET
        # a level as the target: the source stays, the associations go with the target they were made against, exactly
        # as after Context.backproject
        src = ctx.get_source()
        depth.backproject_level(ctx, 1, which=1, fx=fx, cx=cx)
        assert same_bits(ctx.get_source(), src) and code_of(ctx.get_associations) == binding.E_NOT_SET
        # ... and the pyramid is still there
        assert same_bits(depth.pyramid_level(ctx, 2), pm.pyramid(depth.bilateral_host(other), 3)[2])


def test_not_set_and_every_refusal():
    img, K = pm.case("room_37x53")
    a = np.array(img)
    out = np.full(img.shape, 7, np.uint16)
    ap, op = a.ctypes.data_as(U16), out.ctypes.data_as(U16)
    rows, cols = img.shape
    E, NS = binding.E_ARG, binding.E_NOT_SET
    with binding.Context(0) as ctx:
        lib, h = ctx._lib, ctx._h
        r, c = C.c_int32(-5), C.c_int32(-5)
        # before the first build
        assert lib.icpk_depth_pyramid_shape(h, 0, C.byref(r), C.byref(c)) == NS and (r.value, c.value) == (-5, -5)
        assert lib.icpk_depth_pyramid_get(h, 0, op) == NS
        assert lib.icpk_depth_pyramid_backproject(h, 0, 468.6, 318.27, None, 0, -1) == NS
        assert code_of(depth.pyramid_level, ctx, 0) == NS and code_of(depth.backproject_level, ctx, 0) == NS
        ctx.backproject(a, which=0)
        ctx.backproject(a, which=1)
        src, tgt = ctx.get_source(), ctx.get_target()
        # refused builds leave no pyramid behind
        bad = [depth.pyramid_params(**f) for f in (dict(levels=0), dict(levels=9), dict(levels=-1), dict(range_cutoff=0),
                                                   dict(range_cutoff=-1), dict(range_cutoff=65537))]
        for q in bad:
            assert lib.icpk_depth_pyramid_build(h, ap, rows, cols, C.byref(q), None) == E
            assert code_of(depth.build_pyramid, ctx, a, q) == E
        P = C.byref(depth.pyramid_params(range_cutoff=K))
        for f in (dict(radius=0), dict(radius=7), dict(sigma_space=0.0), dict(sigma_range=float("nan")), dict(range_cutoff=4097)):
            assert lib.icpk_depth_pyramid_build(h, ap, rows, cols, P, C.byref(depth.bilateral_params(**f))) == E
        assert lib.icpk_depth_pyramid_build(None, ap, rows, cols, P, None) == E
        assert lib.icpk_depth_pyramid_build(h, None, rows, cols, P, None) == E
        for rr, cc in ((0, cols), (rows, 0), (-1, cols), (1 << 14, (1 << 14) + 1)):
            assert lib.icpk_depth_pyramid_build(h, ap, rr, cc, P, None) == E
        assert lib.icpk_depth_pyramid_shape(h, 0, None, None) == NS
        # with a pyramid: the levels it does not have, and the back-projection's own refusals
        assert depth.build_pyramid(ctx, a, depth.pyramid_params(range_cutoff=K)) == pm.shapes(img.shape, 3)
        keep = levels_of(ctx, 3)
        for level in (-1, 3, 8):
            assert lib.icpk_depth_pyramid_shape(h, level, C.byref(r), C.byref(c)) == E and (r.value, c.value) == (-5, -5)
            assert lib.icpk_depth_pyramid_get(h, level, op) == E
            assert lib.icpk_depth_pyramid_backproject(h, level, 468.6, 318.27, None, 0, -1) == E
        assert lib.icpk_depth_pyramid_shape(None, 0, C.byref(r), C.byref(c)) == E
        assert lib.icpk_depth_pyramid_get(None, 0, op) == E and lib.icpk_depth_pyramid_get(h, 0, None) == E
        assert lib.icpk_depth_pyramid_backproject(None, 0, 468.6, 318.27, None, 0, -1) == E
        for which in (-1, 2):
            assert lib.icpk_depth_pyramid_backproject(h, 1, 468.6, 318.27, None, which, -1) == E
        assert lib.icpk_depth_pyramid_backproject(h, 1, 468.6, 318.27, None, 0, binding.NORMALS_CROSS) == E
        assert lib.icpk_depth_pyramid_backproject(h, 1, 468.6, 318.27, None, 1, binding.NORMALS_REFERENCE + 1) == E
        assert code_of(depth.backproject_level, ctx, 1, which=0, normals_mode=binding.NORMALS_CROSS) == E
        for q in bad:  # a refused build leaves the resident pyramid as it was
            assert lib.icpk_depth_pyramid_build(h, ap, rows, cols, C.byref(q), None) == E
        # a refused call leaves everything as it was
        assert np.all(out == 7) and same_bits(ctx.get_source(), src) and same_bits(ctx.get_target(), tgt)
        assert all(same_bits(x, y) for x, y in zip(levels_of(ctx, 3), keep))
        assert lib.icpk_depth_pyramid_shape(h, 2, None, None) == binding.OK  # (either pointer may be NULL)


# ---- coarse-to-fine tracking ------------------------------------------------------------------------------------------
def noisy_room_frames():
    """the three frames of the TSDF room case with sensor noise: (depth, true pose)"""
    rng = np.random.default_rng(5)
    out = []
    for rot, shift in tc.ROOM_MOTIONS:
        P = tc.pose(rot, shift)
        out.append((synth.render_room_depth(*tc.ROOM_SHAPE, P[:3, :3], P[:3, 3], tc.ROOM_FX, tc.ROOM_CX, 0.002, rng), P))
    return out


@pytest.mark.parametrize("bilateral", [None, True])
def test_model_tracker_with_a_pyramid_is_the_hand_written_loop(ctx, bilateral):
    frames = noisy_room_frames()
    counts = (10, 5, 4)
    kw = dict(max_nn_dist=0.1)
    smooth = depth.bilateral_params() if bilateral else None
    pp = depth.pyramid_params(levels=3)
    vol = TsdfVolume(ctx, **GEOM, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
    tracker = ModelTracker(vol, pose=frames[0][1], step=0.125, bilateral=bilateral, pyramid=counts, **kw)
    poses = [tracker.track(d) for d, _ in frames]
    planes = vol.planes()
    assert tracker.frames == 3 and tracker.levels_skipped == 0 and tracker.pyramid == counts
    assert [st.iterations for st in tracker.level_stats] == list(counts)  # (no threshold: every iteration runs)
    with binding.Context(0) as hand:
        hand.tsdf_create(**GEOM)
        pose, by_hand = frames[0][1].copy(), []
        for k, (d, _) in enumerate(frames):
            if k > 0:
                shapes = depth.build_pyramid(hand, d, pp, smooth=smooth)
                assert shapes == [(120, 160), (60, 80), (30, 40)]
                estimate = pose
                for l in (2, 1, 0):
                    hand.tsdf_raycast(pose, shape=shapes[l], fx=tc.ROOM_FX / 2 ** l, cx=tc.ROOM_CX / 2 ** l, z_near=0.25,
                                      z_far=6.0, step=0.125, min_weight=1)  # the LAST frame's pose at every level
                    hand.tsdf_raycast_to_target()
                    depth.backproject_level(hand, l, which=0, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
                    hand.transform_source(estimate[:3, :3], estimate[:3, 3])
                    hand.commit_source()
                    T, _, _ = hand.align(solve=binding.SOLVE_POINT_TO_PLANE, max_iterations=counts[l], max_nn_dist=0.1 * 2 ** l)
                    estimate = T.astype(np.float64) @ estimate
                pose = estimate
            hand.tsdf_integrate(d, pose, fx=tc.ROOM_FX, cx=tc.ROOM_CX)  # the RAW frame
            by_hand.append(pose.copy())
        want = hand.tsdf_get()
    assert all(same_bits(a, b) for a, b in zip(poses, by_hand))
    assert not np.array_equal(poses[1], frames[0][1]) and not np.array_equal(poses[2], poses[1])
    assert same_bits(planes[0], want[0]) and same_bits(planes[1], want[1])


def test_pyramid_none_and_one_level_are_the_plain_tracker(ctx):
    frames = noisy_room_frames()
    kw = dict(max_iterations=12, max_nn_dist=0.1)

    def run(**extra):
        vol = TsdfVolume(ctx, **GEOM, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
        t = ModelTracker(vol, pose=frames[0][1], step=0.125, **extra)
        return [t.track(d) for d, _ in frames], vol.planes()[:2], t

    plain, plain_planes, t0 = run(**kw)
    none, none_planes, t1 = run(pyramid=None, **kw)
    assert t0.pyramid is None and t1.pyramid is None
    assert all(same_bits(a, b) for a, b in zip(plain, none)) and all(same_bits(a, b) for a, b in zip(plain_planes, none_planes))
    # one level: level 0 is the frame as given, one alignment of 12 iterations through the same gate
    one, one_planes, t2 = run(pyramid=(12,), max_nn_dist=0.1)
    assert t2.pyramid == (12,) and t2.stats.iterations == 12
    assert all(same_bits(a, b) for a, b in zip(plain, one)) and all(same_bits(a, b) for a, b in zip(plain_planes, one_planes))
    assert not np.array_equal(plain[2], plain[1])
    smoothed, _, _ = run(pyramid=(12,), bilateral=True, max_nn_dist=0.1)
    by_k22, _, _ = run(bilateral=True, **kw)
    assert all(same_bits(a, b) for a, b in zip(smoothed, by_k22)) and not same_bits(smoothed[2], plain[2])
    with pytest.raises(ValueError):
        ModelTracker(TsdfVolume(ctx, **GEOM, fx=tc.ROOM_FX, cx=tc.ROOM_CX), pyramid=())


def test_a_level_without_enough_hits_is_skipped(ctx):
    """min_pairs above what the 30 x 40 view can hold: level 2 is skipped and counted, levels 1 and 0 run"""
    frames = noisy_room_frames()
    vol = TsdfVolume(ctx, **GEOM, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
    t = ModelTracker(vol, pose=frames[0][1], step=0.125, pyramid=(10, 5, 4), max_nn_dist=0.1, min_pairs=1500)
    t.track(frames[0][0])
    t.track(frames[1][0])
    assert t.levels_skipped == 1 and t.level_stats[2] is None and t.level_hits[2] < 1500 <= t.level_hits[1]
    assert [t.level_stats[l].iterations for l in (0, 1)] == [10, 5]
    with binding.Context(0) as other:
        vol2 = TsdfVolume(other, **GEOM, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
        t2 = ModelTracker(vol2, pose=frames[0][1], step=0.125, pyramid=(10, 5, 4), max_nn_dist=0.1, min_pairs=30000)
        t2.track(frames[0][0])
        with pytest.raises(RuntimeError):  # only level 0 raises
            t2.track(frames[1][0])
        assert t2.levels_skipped == 2


def pose_error(T, truth):
    E = np.linalg.inv(truth) @ np.asarray(T, np.float64)
    return float(np.degrees(np.arccos(np.clip((np.trace(E[:3, :3]) - 1) / 2, -1, 1)))), float(np.linalg.norm(E[:3, 3]))


BASIN_STEPS = (1, 2, 4, 8)


def test_what_the_pyramid_buys_on_the_room_is_reported(ctx):
    """The model is the three noiseless room frames fused at their true poses.  The next frame is rendered at the last
    pose moved further by s times the motion from it to ROOM_FOURTH (rotation angles and centre, each moved linearly),
    and both trackers start from the last true pose: the plain one with 19 iterations, the pyramid with (10, 5, 4),
    both through max_nn_dist = 0.1.  Printed for DESIGN.md (K24).  The yardstick is the unchanged plain path and the
    volume's own voxel (0.0625 m)."""
    c = tc.case("room")
    (r3, t3), (r4, t4) = tc.ROOM_MOTIONS[2], tc.ROOM_FOURTH
    P3 = tc.pose(r3, t3)
    vol = TsdfVolume(ctx, **GEOM, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
    for d, P, _ in c["frames"]:
        vol.integrate(d, P)
    model = vol.planes()[:2]
    table = []
    for s in BASIN_STEPS:
        rot = tuple(a + s * (b - a) for a, b in zip(r3, r4))
        shift = tuple(a + s * (b - a) for a, b in zip(t3, t4))
        d, truth = tc.room_frame(rot, shift)
        row = [s]
        for extra in (dict(max_iterations=19), dict(pyramid=(10, 5, 4))):
            vol.set_planes(*model)
            t = ModelTracker(vol, pose=P3, step=0.125, max_nn_dist=0.1, **extra)
            t.frames = 3  # (the model holds three frames: this one is aligned against it)
            row += pose_error(t.track(d), truth)
        table.append(row)
        print(f"s = {s}: moved {pose_error(P3, truth)[0]:.2f} deg {1000 * pose_error(P3, truth)[1]:.1f} mm; plain "
              f"{row[1]:.4f} deg {1000 * row[2]:.2f} mm; pyramid (10, 5, 4) {row[3]:.4f} deg {1000 * row[4]:.2f} mm")
    voxel = tc.ROOM_VOLUME["voxel"]
    separating = [row[0] for row in table if row[2] > voxel and row[4] < voxel / 4]
    print(f"steps at which the plain tracker is off by more than a voxel and the pyramid by less than a quarter: {separating}")
    # Measured on an MI355X (has the table): both trackers end within 6 mm of the truth at s = 1 and 2
    # and both are lost at s = 4 and 8, so no s separates them on this scene and nothing is asserted about the basin.
    assert all(np.isfinite(v) for row in table for v in row)
