"""K26 on the device: the intensity pyramid, the view's colour gradients and the joint projective reduction against
tests/projective_color_model.py byte for byte on the cases of tests/projective_color_cases.py; the coloured loop by its
trace, as K25's tests do it; the early stops; lifetimes, refusals and what the calls leave alone;
tsdf.ModelTracker(projective_color=...) against the loop written out by hand; the wall the feature is for, held to twice
the figures the numpy models reached before anything ran on a device; and the room tables, printed for DESIGN.md."""
import ctypes as C
import functools

import numpy as np
import pytest

import color_model as cm
import projective_cases as pc
import projective_color_cases as kc
import projective_color_model as km
import projective_model as jm
import tsdf_cases as tc
from icp_slam_prototype_amd import binding, depth, synth
from icp_slam_prototype_amd.tsdf import ModelTracker, TsdfVolume

pytestmark = pytest.mark.gpu

GEOM = {k: tc.ROOM_VOLUME[k] for k in ("dims", "voxel", "origin", "trunc")}
VOXEL = tc.ROOM_VOLUME["voxel"]


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


def pose_error(T, truth):
    E = np.linalg.inv(truth) @ np.asarray(T, np.float64)
    return float(np.degrees(np.arccos(np.clip((np.trace(E[:3, :3]) - 1) / 2, -1, 1)))), float(np.linalg.norm(E[:3, 3]))


# ---- the intensity pyramid --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", kc.PYRAMID_CASES)
def test_intensity_pyramid_gives_the_models_bytes(ctx, name):
    d, inten, K, levels = kc.pyramid_case(name)
    want = kc.pyramid_expected(name)
    shapes = depth.build_pyramid(ctx, d, depth.pyramid_params(levels=levels, range_cutoff=K), intensity=inten)
    for l in range(levels):
        got = binding.pyramid_intensity(ctx, l)
        assert got.shape == shapes[l] and same_bits(got, np.array(want[l])), (name, l)
    # a second setting gives the same bytes, and the depth pyramid is untouched
    before = [depth.pyramid_level(ctx, l).tobytes() for l in range(levels)]
    binding.set_pyramid_intensity(ctx, inten)
    assert all(same_bits(binding.pyramid_intensity(ctx, l), np.array(want[l])) for l in range(levels))
    assert [depth.pyramid_level(ctx, l).tobytes() for l in range(levels)] == before


def test_intensity_pyramid_beside_the_smoothed_depth(ctx):
    """with `smooth` the depth levels are the smoothed ones and the intensity is not smoothed: the model over the depth
    levels the device holds"""
    d, inten, K, _ = kc.pyramid_case("room_color_masked")
    depth.build_pyramid(ctx, d, depth.pyramid_params(levels=3), smooth=depth.bilateral_params(), intensity=inten)
    levels = [depth.pyramid_level(ctx, l) for l in range(3)]
    assert not same_bits(levels[0], np.array(d))
    want = np.array(inten)
    assert same_bits(binding.pyramid_intensity(ctx, 0), want)
    for l in (1, 2):
        want = km.intensity_level_up(levels[l - 1], want, K)
        assert same_bits(binding.pyramid_intensity(ctx, l), want)


def test_intensity_pyramid_lifetime_and_refusals():
    E, NS = binding.E_ARG, binding.E_NOT_SET
    d, inten, K, _ = kc.pyramid_case("17x65")
    with binding.Context(0) as x:
        assert code_of(binding.set_pyramid_intensity, x, inten) == NS and code_of(binding.pyramid_intensity, x, 0) == NS
        depth.build_pyramid(x, d, depth.pyramid_params(levels=3))
        assert code_of(binding.pyramid_intensity, x, 0) == NS  # a pyramid without intensity levels
        binding.set_pyramid_intensity(x, inten)
        good = [binding.pyramid_intensity(x, l) for l in range(3)]
        assert code_of(binding.pyramid_intensity, x, 3) == E and code_of(binding.pyramid_intensity, x, -1) == E
        assert code_of(binding.set_pyramid_intensity, x, np.array(inten)[:, :-1]) == E  # not level 0's shape
        assert code_of(binding.set_pyramid_intensity, x, np.array(inten).T) == E
        for bad in (np.nan, np.inf, -1e-6, 1.0001):
            ii = np.array(inten)
            ii[16, 64] = bad
            assert code_of(binding.set_pyramid_intensity, x, ii) == E
        assert x._lib.icpk_depth_pyramid_set_intensity(x._h, None, 17, 65) == E
        assert x._lib.icpk_depth_pyramid_get_intensity(x._h, 0, None) == E
        # a refused call has left everything as it was
        assert all(same_bits(binding.pyramid_intensity(x, l), good[l]) for l in range(3))
        depth.build_pyramid(x, d, depth.pyramid_params(levels=3))  # the next build drops the intensity levels
        assert code_of(binding.pyramid_intensity, x, 0) == NS
        depth.build_pyramid(x, d, depth.pyramid_params(levels=2), intensity=inten)
        assert same_bits(binding.pyramid_intensity(x, 1), good[1]) and code_of(binding.pyramid_intensity, x, 2) == E


# ---- the view gradients -----------------------------------------------------------------------------------------------
def cast(c, g):
    kc.create_volume(c, binding, g["volume"])
    c.tsdf_raycast(g["pose"], **g["view"])


@pytest.mark.parametrize("name", kc.GRADIENT_CASES)
def test_view_gradients_give_the_models_bytes(ctx, name):
    g = kc.gradient_case(name)
    cast(ctx, g)
    view = ctx.tsdf_get_raycast()
    maps = np.concatenate([view["points"], view["normals"], view["depth"][None], view["intensity"][None]])
    assert maps.tobytes() == g["maps"].tobytes()  # (the inputs the device holds are the model's)
    binding.raycast_color_gradients(ctx, g["radius"], g["min_neighbors"], keep_sums=True)
    grad, S = binding.get_raycast_color_gradients(ctx, sums=True)
    assert S.reshape(-1, 10).tobytes() == g["sums"].tobytes()
    assert same_bits(grad, np.array(g["gradients"]))
    assert same_bits(cm.gradients_from_sums(S.reshape(-1, 10), maps[3:6].reshape(3, -1), g["radius"], g["min_neighbors"]),
                     np.array(g["gradients"]).reshape(3, -1))
    # a second run gives the same bytes; without the flag the sums are gone; the maps are untouched
    binding.raycast_color_gradients(ctx, g["radius"], g["min_neighbors"])
    assert same_bits(binding.get_raycast_color_gradients(ctx), grad)
    assert code_of(binding.get_raycast_color_gradients, ctx, sums=True) == binding.E_NOT_SET
    again = ctx.tsdf_get_raycast()
    assert all(again[k].tobytes() == view[k].tobytes() for k in ("points", "normals", "depth", "intensity"))


def test_the_gradient_cases_hold_their_conditions():
    kc.check_gradient_conditions()


def test_view_gradient_lifetime_and_refusals():
    E, NS = binding.E_ARG, binding.E_NOT_SET
    g = kc.gradient_case("7x9")
    with binding.Context(0) as x:
        assert code_of(binding.raycast_color_gradients, x, 0.1) == NS  # no volume
        v = tc.case("room")["volume"]
        x.tsdf_create(dims=v["dims"], voxel=v["voxel"], origin=v["origin"], trunc=v["trunc"])
        assert code_of(binding.raycast_color_gradients, x, 0.1) == NS  # no ray cast
        x.tsdf_raycast(g["pose"], **g["view"])
        assert code_of(binding.raycast_color_gradients, x, 0.1) == E  # a volume without colour
        assert code_of(binding.get_raycast_color_gradients, x) == NS
        cast(x, g)
        assert code_of(binding.get_raycast_color_gradients, x) == NS  # a ray cast without gradients
        binding.raycast_color_gradients(x, g["radius"], g["min_neighbors"], keep_sums=True)
        good = binding.get_raycast_color_gradients(x, sums=True)
        for r in (0.0, -1.0, np.nan, np.inf):
            assert code_of(binding.raycast_color_gradients, x, r) == E
        assert code_of(binding.raycast_color_gradients, x, 0.1, 0) == E
        assert x._lib.icpk_tsdf_raycast_color_gradients(x._h, 0.1, 4, 2) == E  # an unknown flag
        assert x._lib.icpk_tsdf_get_raycast_color_gradient_sums(x._h, None) == E
        # a refused call has left everything as it was
        now = binding.get_raycast_color_gradients(x, sums=True)
        assert same_bits(now[0], good[0]) and same_bits(now[1], good[1])
        # NULL planes are allowed
        assert x._lib.icpk_tsdf_get_raycast_color_gradients(x._h, None, None, None) == binding.OK
        x.tsdf_raycast(g["pose"], **g["view"])  # the next ray cast drops the gradients and the kept sums
        assert code_of(binding.get_raycast_color_gradients, x) == NS
        assert x._lib.icpk_tsdf_get_raycast_color_gradient_sums(x._h, good[1].ctypes.data_as(C.POINTER(C.c_int64))) == NS
        binding.raycast_color_gradients(x, g["radius"], g["min_neighbors"])
        assert same_bits(binding.get_raycast_color_gradients(x), good[0])
        x.tsdf_reset()  # ... and so does everything that drops the maps
        assert code_of(binding.get_raycast_color_gradients, x) == NS and code_of(binding.raycast_color_gradients, x, 0.1) == NS


# ---- the joint reduction ----------------------------------------------------------------------------------------------
def test_the_cases_accept_what_k25_accepts():
    kc.check_conditions()


@pytest.mark.parametrize("name", kc.NAMES)
def test_colored_reduce_gives_the_models_bytes(ctx, name):
    c = kc.case(name)
    p = kc.device_setup(ctx, name, depth, binding)
    # (the inputs the device holds are the model's: the rest compares the rule alone)
    assert same_bits(depth.pyramid_level(ctx, c["level"]), np.array(c["level_image"]))
    assert same_bits(binding.pyramid_intensity(ctx, c["level"]), np.array(c["level_intensity"]))
    assert same_bits(binding.get_raycast_color_gradients(ctx), np.array(kc.gradients_of(name)))
    k25 = pc.expected(name)
    for lam in kc.LAMBDAS:
        want = kc.expected(name, lam)
        sums, count = binding.projective_reduce_colored(ctx, c["estimate"], p, dict(lambda_geometric=lam))
        assert count == want["count"] == k25["count"], lam  # counts are K25's
        assert sums.tobytes() == want["sums"].tobytes(), lam
    # at 1 the sums are icpk_projective_reduce's bytes on the same inputs; the codes are K25's
    geo, n = binding.projective_reduce(ctx, c["estimate"], p)
    assert n == count and geo.tobytes() == sums.tobytes()
    pixel, _ = binding.projective_associate(ctx, c["estimate"], p)
    assert pixel.reshape(-1).tobytes() == k25["pixel"].tobytes()


def run_loop(c, name, color=None, **kw):
    p = kc.device_setup(c, name, depth, binding)
    for k, v in kw.items():
        setattr(p, k, v)
    pose, res = binding.align_projective_colored(c, kc.case(name)["estimate"], p, color)
    return pose, res, binding.projective_trace(c)


@pytest.mark.parametrize("name", kc.LOOP_CASES)
def test_the_colored_loop_by_its_trace(ctx, name):
    c = kc.case(name)
    pose, res, trace = run_loop(ctx, name, max_iterations=10)
    assert (res.status, res.iterations, len(trace)) == (binding.OK, 10, 10)
    assert trace[0]["pose"].tobytes() == c["estimate"][:3].tobytes()  # E_0 is the input, bit for bit
    worst = 0.0
    for k, it in enumerate(trace):
        assert it["status"] == binding.OK
        E = np.vstack([it["pose"], [0, 0, 0, 1]])
        px = km.pixels(**kc.model_args(name, pose=E))
        sums, count = km.reduce(px["terms"], px["pixel"])
        assert it["count"] == count, k
        assert it["sums"].tobytes() == sums.tobytes(), k  # the model's bytes AT the recorded pose
        status, En = jm.update(it["sums"], it["count"], E)
        nxt = trace[k + 1]["pose"] if k + 1 < len(trace) else pose[:3]
        assert status == jm.OK
        worst = max(worst, float(np.abs(En[:3] - nxt).max()))
    print(f"{name}: largest |E_(k+1) - model's update of E_k| over 10 coloured iterations: {worst:.3e}")
    assert worst < 1e-12
    assert pose[3].tolist() == [0, 0, 0, 1]
    assert res.count == trace[-1]["count"] and res.mean_dist == trace[-1]["sums"][27] / trace[-1]["count"]
    # the coloured loop is not the geometric one
    geo, _ = binding.align_projective(ctx, c["estimate"], level=c["level"], fx=c["fx"], cx=c["cx"], max_iterations=10)
    assert geo.tobytes() != pose.tobytes()


def test_early_stops(ctx):
    c = kc.case("room_l0")
    few = kc.expected("room_l0")["count"] + 1
    pose, res, trace = run_loop(ctx, "room_l0", max_iterations=5, min_pairs=few)
    assert (res.status, res.iterations, len(trace)) == (binding.W_TOO_FEW_PAIRS, 0, 1)
    assert pose.tobytes() == c["estimate"].tobytes() and trace[0]["status"] == binding.W_TOO_FEW_PAIRS
    assert res.count == few - 1 and trace[0]["sums"].tobytes() == kc.expected("room_l0")["sums"].tobytes()
    # every pixel BEHIND: no pair
    c = kc.case("plane_behind")
    pose, res, trace = run_loop(ctx, "plane_behind", max_iterations=4)
    assert (res.status, res.iterations, res.count, res.mean_dist, len(trace)) == (binding.W_TOO_FEW_PAIRS, 0, 0, 0.0, 1)
    assert pose.tobytes() == c["estimate"].tobytes()
    # the fronto-parallel plane with the photometric term switched off is K25's degenerate case; E stays
    c = kc.case("plane")
    pose, res, trace = run_loop(ctx, "plane", dict(lambda_geometric=1.0), max_iterations=4)
    assert (res.status, res.iterations, len(trace)) == (binding.W_DEGENERATE, 0, 1)
    assert pose.tobytes() == c["estimate"].tobytes() and res.count == kc.expected("plane")["count"] == 432
    # ... and with it the same plane, textured, is not
    pose, res, trace = run_loop(ctx, "plane", max_iterations=4)
    assert (res.status, res.iterations, len(trace)) == (binding.OK, 4, 4)


def snapshot(c, levels):
    """what the coloured calls must leave alone: the clouds, the associations, the maps, the gradients, both pyramids, the
    volume"""
    idx, dist = c.get_associations()
    view = c.tsdf_get_raycast()
    return [c.get_source().tobytes(), c.get_target().tobytes(), c.get_target_normals().tobytes(), idx.tobytes(), dist.tobytes()] + \
        [view[k].tobytes() for k in ("points", "normals", "depth", "intensity")] + [binding.get_raycast_color_gradients(c).tobytes()] + \
        [depth.pyramid_level(c, l).tobytes() for l in range(levels)] + [binding.pyramid_intensity(c, l).tobytes() for l in range(levels)] + \
        [a.tobytes() for a in c.tsdf_get(intensity=True)]


def test_the_context_is_left_alone(ctx):
    """After any of the coloured calls the source, target, associations, maps, gradients, pyramids and volume are the
    bytes from before; an icpk_align and an icpk_align_projective behind them give what they give on a context that never
    made them; two calls in a row give the same bytes; and a context with a history gives a fresh context's bytes."""
    name = "room_l1"
    c = kc.case(name)
    d3 = tc.case("room")["frames"][2][0]
    kw = dict(solve=binding.SOLVE_POINT_TO_PLANE, max_iterations=4, max_nn_dist=0.1)

    def clouds(x):
        x.backproject_with_normals(d3, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
        x.set_source(synth.backproject(c["depth"], None, tc.ROOM_FX, tc.ROOM_CX))

    def calls(x, p):
        return [binding.align_projective_colored(x, c["estimate"], p), binding.projective_trace(x),
                binding.projective_reduce_colored(x, c["estimate"], p)]

    with binding.Context(0) as fresh:
        p = kc.device_setup(fresh, name, depth, binding)
        want = calls(fresh, p)
    with binding.Context(0) as plain:  # never makes a coloured call
        clouds(plain)
        T0, st0, _ = plain.align(**kw)
        assoc0 = plain.get_associations()
        p = kc.device_setup(plain, name, depth, binding)
        geo0 = binding.align_projective(plain, c["estimate"], p)
    clouds(ctx)
    ctx.align(**kw)
    kc.device_setup(ctx, "17x19", depth, binding)
    p = kc.device_setup(ctx, name, depth, binding)
    clouds(ctx)
    ctx.nn()
    before = snapshot(ctx, 2)
    got = calls(ctx, p)
    again = calls(ctx, p)
    assert snapshot(ctx, 2) == before

    def blob(r):
        (pose, res), trace, (sums, count) = r
        return [pose.tobytes(), bytes(res), sums.tobytes(), count] + \
            [t["pose"].tobytes() + t["sums"].tobytes() + bytes([t["status"]]) + str(t["count"]).encode() for t in trace]

    assert blob(got) == blob(want) and blob(again) == blob(want)
    geo1 = binding.align_projective(ctx, c["estimate"], p)
    assert geo1[0].tobytes() == geo0[0].tobytes() and bytes(geo1[1]) == bytes(geo0[1])
    T1, st1, _ = ctx.align(**kw)
    assoc1 = ctx.get_associations()
    assert same_bits(T1, T0) and st1.final_pairs == st0.final_pairs and st1.final_mse == st0.final_mse
    assert same_bits(assoc1[0], assoc0[0]) and same_bits(assoc1[1], assoc0[1])


def test_not_set_and_every_refusal():
    name = "room_l1"
    c = kc.case(name)
    E, NS = binding.E_ARG, binding.E_NOT_SET
    P = c["estimate"]
    calls = lambda x: tuple(functools.partial(f, x) for f in (binding.align_projective_colored, binding.projective_reduce_colored))
    with binding.Context(0) as x:
        for call in calls(x):
            assert code_of(call, P) == NS  # no volume
        v = tc.case("room")["volume"]
        x.tsdf_create(dims=v["dims"], voxel=v["voxel"], origin=v["origin"], trunc=v["trunc"])
        for call in calls(x):
            assert code_of(call, P) == NS  # no ray cast
        x.tsdf_raycast(c["view_pose"], **c["view"])
        for call in calls(x):
            assert code_of(call, P) == NS  # no pyramid
        depth.build_pyramid(x, c["depth"], depth.pyramid_params(levels=2), intensity=c["intensity"])
        for call in calls(x):
            assert code_of(call, P, level=1, fx=c["fx"], cx=c["cx"]) == E  # a volume without colour
        p = kc.device_setup(x, name, depth, binding, gradients=False)
        for call in calls(x):
            assert code_of(call, P, p) == NS  # no view gradients for this ray cast
        p = kc.device_setup(x, name, depth, binding, intensity=False)
        for call in calls(x):
            assert code_of(call, P, p) == NS  # no intensity pyramid
        p = kc.device_setup(x, name, depth, binding)
        good = binding.align_projective_colored(x, P, p)
        trace = binding.projective_trace(x)
        bad = P.copy()
        bad[0, 3] = np.nan
        for call in calls(x):
            assert code_of(call, bad, p) == E
            for lam in (np.nan, np.inf, -0.001, 1.001):
                assert code_of(call, P, p, dict(lambda_geometric=lam)) == E, lam
            for kw in (dict(level=2), dict(level=-1), dict(fx=0.0), dict(fx=np.inf), dict(cx=np.nan), dict(max_dist=0.0),
                       dict(max_dist=np.nan), dict(min_pairs=0), dict(max_iterations=0), dict(max_iterations=65)):
                assert code_of(call, P, level=kw.get("level", 1), **{k: v for k, v in kw.items() if k != "level"}) == E, kw
        lib, h = x._lib, x._h
        assert lib.icpk_align_projective_colored(h, C.byref(p), None, None, None, None) == E
        # a refused call has left everything as it was
        t2 = binding.projective_trace(x)
        assert len(t2) == len(trace) == 10 and all(a["sums"].tobytes() == b["sums"].tobytes() for a, b in zip(t2, trace))
        again = binding.align_projective_colored(x, P, p)
        assert again[0].tobytes() == good[0].tobytes() and bytes(again[1]) == bytes(good[1])
        # NULL colour parameters are the defaults, NULL outputs are allowed
        assert lib.icpk_align_projective_colored(h, C.byref(p), None, P.ctypes.data_as(C.POINTER(C.c_double)), None, None) == binding.OK
        assert all(a["sums"].tobytes() == b["sums"].tobytes() for a, b in zip(binding.projective_trace(x), trace))
        x.tsdf_raycast(c["view_pose"], **c["view"])  # a new ray cast: its gradients are not made yet
        for call in calls(x):
            assert code_of(call, P, p) == NS
        x.tsdf_reset()
        for call in calls(x):
            assert code_of(call, P, p) == NS  # the reset volume has no ray cast


# ---- the tracker ------------------------------------------------------------------------------------------------------
def noisy_room_frames():
    """the three frames of the colour room case with sensor noise: (depth, true pose, intensity)"""
    rng = np.random.default_rng(5)
    out = []
    for rot, shift in tc.ROOM_MOTIONS:
        P = tc.pose(rot, shift)
        out.append((synth.render_room_depth(*tc.ROOM_SHAPE, P[:3, :3], P[:3, 3], tc.ROOM_FX, tc.ROOM_CX, 0.002, rng), P,
                    tc.room_intensity(rot, shift)))
    return out


@pytest.mark.parametrize("counts", [(10, 5, 4), None])
def test_model_tracker_projective_color_is_the_hand_written_loop(ctx, counts):
    frames = noisy_room_frames()
    levels = 1 if counts is None else len(counts)
    iters = (7,) if counts is None else counts
    kw = dict(max_iterations=7) if counts is None else dict(pyramid=counts)
    vol = TsdfVolume(ctx, **GEOM, color=True, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
    tracker = ModelTracker(vol, pose=frames[0][1], step=0.125, projective=True, projective_color=True, **kw)
    poses = [tracker.track(d, i) for d, _, i in frames]
    planes = vol.planes(intensity=True)
    assert tracker.frames == 3 and tracker.levels_skipped == 0
    assert [st.iterations for st in tracker.level_stats] == list(iters) and all(st.status == binding.OK for st in tracker.level_stats)
    with binding.Context(0) as hand:
        hand.tsdf_create(**GEOM, flags=binding.TSDF_COLOR)
        pose, by_hand = frames[0][1].copy(), []
        for k, (d, _, inten) in enumerate(frames):
            if k > 0:
                shapes = depth.build_pyramid(hand, d, depth.pyramid_params(levels=levels))
                binding.set_pyramid_intensity(hand, inten)  # one upload per frame, after the build
                estimate = pose
                for l in range(levels - 1, -1, -1):
                    hand.tsdf_raycast(pose, shape=shapes[l], fx=tc.ROOM_FX / 2 ** l, cx=tc.ROOM_CX / 2 ** l, z_near=0.25, z_far=6.0,
                                      step=0.125, min_weight=1)
                    binding.raycast_color_gradients(hand, 2 * VOXEL * 2 ** l, 4)
                    estimate, _ = binding.align_projective_colored(hand, estimate, level=l, fx=tc.ROOM_FX, cx=tc.ROOM_CX,
                                                                   max_iterations=iters[l], max_dist=0.5)
                pose = estimate
            hand.tsdf_integrate(d, pose, inten, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
            by_hand.append(pose.copy())
        want = hand.tsdf_get(intensity=True)
    assert all(same_bits(a, b) for a, b in zip(poses, by_hand))
    assert not np.array_equal(poses[1], frames[0][1]) and not np.array_equal(poses[2], poses[1])
    assert all(same_bits(planes[k], want[k]) for k in range(3))


def test_projective_color_none_is_the_tracker_as_it_was(ctx):
    frames = noisy_room_frames()

    def run(**extra):
        vol = TsdfVolume(ctx, **GEOM, color=True, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
        t = ModelTracker(vol, pose=frames[0][1], step=0.125, projective=True, **extra)
        return [t.track(d, i) for d, _, i in frames], vol.planes(intensity=True), t

    for extra in (dict(max_iterations=7), dict(pyramid=(10, 5, 4)), dict(pyramid=(6, 3), bilateral=True)):
        a, pa, ta = run(**extra)
        b, pb, tb = run(projective_color=None, **extra)
        assert tb.projective_color is None and ta.projective_color is None
        assert all(same_bits(x, y) for x, y in zip(a, b)) and all(same_bits(x, y) for x, y in zip(pa, pb))
        with binding.Context(0) as hand:  # ... and both are K25's hand-written loop: today's bytes
            hand.tsdf_create(**GEOM, flags=binding.TSDF_COLOR)
            levels = len(extra.get("pyramid", (0,)))
            iters = extra.get("pyramid", (7,))
            pose = frames[0][1].copy()
            for k, (d, _, inten) in enumerate(frames):
                if k > 0:
                    shapes = depth.build_pyramid(hand, d, depth.pyramid_params(levels=levels),
                                                 smooth=depth.bilateral_params() if extra.get("bilateral") else None)
                    estimate = pose
                    for l in range(levels - 1, -1, -1):
                        hand.tsdf_raycast(pose, shape=shapes[l], fx=tc.ROOM_FX / 2 ** l, cx=tc.ROOM_CX / 2 ** l, z_near=0.25,
                                          z_far=6.0, step=0.125, min_weight=1)
                        estimate, _ = binding.align_projective(hand, estimate, level=l, fx=tc.ROOM_FX, cx=tc.ROOM_CX,
                                                               max_iterations=iters[l], max_dist=0.5)
                    pose = estimate
                hand.tsdf_integrate(d, pose, inten, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
                assert same_bits(pose, a[k])
    # with bilateral the coloured tracker smooths the depth and not the intensity: the level-0 intensity is the frame's
    vol = TsdfVolume(ctx, **GEOM, color=True, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
    t = ModelTracker(vol, pose=frames[0][1], step=0.125, projective=True, projective_color=True, bilateral=True, pyramid=(6, 3))
    t.track(frames[0][0], frames[0][2])
    t.track(frames[1][0], frames[1][2])
    assert same_bits(binding.pyramid_intensity(ctx, 0), frames[1][2]) and not same_bits(depth.pyramid_level(ctx, 0), frames[1][0])
    # what the constructor and track refuse
    plain = TsdfVolume(ctx, **GEOM, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
    with pytest.raises(ValueError, match="colour volume"):
        ModelTracker(plain, projective=True, projective_color=True)
    vol = TsdfVolume(ctx, **GEOM, color=True, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
    with pytest.raises(ValueError, match="needs projective"):
        ModelTracker(vol, projective_color=True)
    with pytest.raises(ValueError, match="no setting"):
        ModelTracker(vol, projective=True, projective_color=dict(radius=1.0))
    t = ModelTracker(vol, pose=frames[0][1], projective=True, projective_color=dict(lambda_geometric=0.9, gradient_radius=0.2, min_neighbors=3))
    with pytest.raises(ValueError, match="intensity"):
        t.track(frames[0][0])
    assert t.frames == 0


# ---- the evidence -----------------------------------------------------------------------------------------------------
def test_the_wall(ctx):
    """The claim the feature makes, on the device: an exact fronto-parallel textured plane fused into a colour volume at
    frame 0's true pose; frame 1 from a camera moved in the plane by (30, -20) mm, 4 mm along the normal and 1 degree
    about it; tracking starts at frame 0's pose, 20 iterations at level 0.  The numpy models reached rotation
    (Frobenius) 5.54e-4 and translation 4.98 mm (projective_color_cases.WALL_MEASURED, below the 9 mm the claim stands
    on); the assertion is twice those figures.  The geometric icpk_align_projective on the same inputs stops with
    ICPK_W_DEGENERATE (in the models and here) or leaves more than half the in-plane motion."""
    w = kc.wall()
    (d0, i0), (d1, i1) = w["frames"]
    P0, P1 = w["poses"]
    kc.create_volume(ctx, binding, "wall")
    ctx.tsdf_raycast(P0, **kc.WALL_VIEW)
    binding.raycast_color_gradients(ctx, kc.WALL_RADIUS, kc.WALL_MIN_NB)
    depth.build_pyramid(ctx, d1, depth.pyramid_params(levels=1), intensity=i1)
    p = binding.default_projective_params(level=0, fx=kc.WALL_FX, cx=kc.WALL_CX, max_iterations=kc.WALL_ITER, max_dist=kc.WALL_MAX_DIST)
    pose, res = binding.align_projective_colored(ctx, P0, p)
    rot, trans = kc.wall_errors(pose)
    print(f"wall, device: coloured {rot:.6e} / {1000 * trans:.4f} mm after {res.iterations} iterations, {res.count} pairs")
    assert res.status == binding.OK and res.iterations == kc.WALL_ITER
    assert kc.WALL_MEASURED[1] < kc.WALL_CONDITION
    assert rot <= 2 * kc.WALL_MEASURED[0] and trans <= 2 * kc.WALL_MEASURED[1]
    # the models' own loop ends where the device's does
    assert np.abs(kc.wall_model()["colored"]["pose"] - pose).max() < 1e-6
    geo, gres = binding.align_projective(ctx, P0, p)
    in_plane = float(np.linalg.norm(geo[:2, 3] - P1[:2, 3]))
    print(f"wall, device: geometric status {gres.status}, iterations {gres.iterations}, in-plane error {1000 * in_plane:.2f} mm")
    assert gres.status == binding.W_DEGENERATE or in_plane > 0.5 * float(np.hypot(0.030, 0.020))
    # the tracker over the same two frames
    vol = TsdfVolume(ctx, **{k: kc.WALL_VOLUME[k] for k in ("dims", "voxel", "origin", "trunc")}, color=True, fx=kc.WALL_FX, cx=kc.WALL_CX)
    t = ModelTracker(vol, pose=P0, z_near=0.25, z_far=3.0, step=0.05, projective=True, projective_color=True, max_iterations=kc.WALL_ITER)
    t.track(d0, i0)
    assert same_bits(t.track(d1, i1), pose)


def test_the_room_tables(ctx):
    """K25's tracking table (every frame placed by its predecessor's true pose, the model built from the tracker's own
    estimates, 20 iterations) and its basin table (s = 1 .. 4, 19 iterations) on room_color, geometric and coloured side
    by side, printed for DESIGN.md.  The room's texture is step-edged rectangles seen through 62.5 mm voxels: the numpy
    models showed the coloured tracker OUTSIDE K25's quarter-voxel bar (DESIGN.md K26 has the table), so nothing is
    asserted on the coloured column; the geometric column must still meet K25's bar on the colour volume."""
    c = tc.case("room_color")
    d4, P4 = tc.room_frame(*tc.ROOM_FOURTH)
    frames = [(d, P, i) for d, P, i in c["frames"]] + [(d4, P4, tc.room_intensity(*tc.ROOM_FOURTH))]
    for color in (None, True):
        vol = TsdfVolume(ctx, **GEOM, color=True, fx=c["fx"], cx=c["cx"])
        tracker = ModelTracker(vol, pose=frames[0][1], z_near=0.25, z_far=6.0, step=0.125, projective=dict(max_dist=0.5),
                               projective_color=color, max_iterations=20)
        for k, (d, P, inten) in enumerate(frames):
            if k > 0:
                tracker.pose = frames[k - 1][1].copy()
            e = pose_error(tracker.track(d, inten), P)
            print(f"{'coloured' if color else 'geometric'} frame {k}: {e[0]:.4f} deg, {1000 * e[1]:.2f} mm")
    (r3, t3), (r4, t4) = tc.ROOM_MOTIONS[2], tc.ROOM_FOURTH
    P3 = tc.pose(r3, t3)
    vol = TsdfVolume(ctx, **GEOM, color=True, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
    for d, P, inten in c["frames"]:
        vol.integrate(d, P, inten)
    model = vol.planes(intensity=True)
    for s in (1, 2, 3, 4):
        rot = tuple(a + s * (b - a) for a, b in zip(r3, r4))
        shift = tuple(a + s * (b - a) for a, b in zip(t3, t4))
        d, truth = tc.room_frame(rot, shift)
        inten = tc.room_intensity(rot, shift)
        row = []
        for color in (None, True):
            vol.set_planes(*model)
            t = ModelTracker(vol, pose=P3, step=0.125, max_iterations=19, projective=dict(max_dist=0.5), projective_color=color)
            t.frames = 3
            row += pose_error(t.track(d, inten), truth)
        print(f"s = {s}: geometric {row[0]:.4f} deg {1000 * row[1]:.2f} mm; coloured {row[2]:.4f} deg {1000 * row[3]:.2f} mm")
        assert row[1] < VOXEL / 4, row
