"""K25 on the device: icpk_projective_associate / _reduce against tests/projective_model.py byte for byte on every case of
tests/projective_cases.py; the loop by its trace (the recorded sums are the model's bytes AT the recorded pose, and the
next pose is the model's update of it from those sums); the early stops; what the calls leave alone; the refusals;
tsdf.ModelTracker(projective=...) against the loop written out by hand; and tracking on the room scene against the
project's own yardsticks (K20's four frames, K24's basin), with the tables printed for DESIGN.md."""
import ctypes as C
import functools

import numpy as np
import pytest

import projective_cases as pc
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


def test_the_cases_hold_their_condition_before_anything_runs():
    pc.check_conditions()


@pytest.mark.parametrize("name", pc.NAMES)
def test_associate_and_reduce_give_the_models_bytes(ctx, name):
    c, want = pc.case(name), pc.expected(name)
    p = pc.device_setup(ctx, name, depth, binding)
    # (the inputs the device holds are the model's: the rest compares the rule alone)
    assert same_bits(depth.pyramid_level(ctx, c["level"]), np.array(c["level_image"]))
    view = ctx.tsdf_get_raycast()
    assert np.concatenate([view["points"], view["normals"], view["depth"][None]]).tobytes() == pc.maps_of(name)[:7].tobytes()
    pixel, dist = binding.projective_associate(ctx, c["estimate"], p)
    assert pixel.shape == dist.shape == c["level_image"].shape
    assert pixel.reshape(-1).tobytes() == want["pixel"].tobytes()
    assert dist.reshape(-1).tobytes() == want["dist"].tobytes()
    sums, count = binding.projective_reduce(ctx, c["estimate"], p)
    assert count == want["count"]
    assert sums.tobytes() == want["sums"].tobytes()


def run_loop(c, name, **kw):
    p = pc.device_setup(c, name, depth, binding)
    for k, v in kw.items():
        setattr(p, k, v)
    pose, res = binding.align_projective(c, pc.case(name)["estimate"], p)
    return pose, res, binding.projective_trace(c)


@pytest.mark.parametrize("name", pc.LOOP_CASES)
def test_the_loop_by_its_trace(ctx, name):
    c = pc.case(name)
    pose, res, trace = run_loop(ctx, name, max_iterations=10)
    assert (res.status, res.iterations, len(trace)) == (binding.OK, 10, 10)
    assert trace[0]["pose"].tobytes() == c["estimate"][:3].tobytes()  # E_0 is the input, bit for bit
    worst = 0.0
    for k, it in enumerate(trace):
        assert it["status"] == binding.OK
        E = np.vstack([it["pose"], [0, 0, 0, 1]])
        px = jm.pixels(**pc.model_args(name, pose=E))
        sums, count = jm.reduce(px["terms"], px["pixel"])
        assert it["count"] == count, k
        assert it["sums"].tobytes() == sums.tobytes(), k  # the model's bytes AT the recorded pose
        status, En = jm.update(it["sums"], it["count"], E)
        nxt = trace[k + 1]["pose"] if k + 1 < len(trace) else pose[:3]
        assert status == jm.OK
        worst = max(worst, float(np.abs(En[:3] - nxt).max()))
    print(f"{name}: largest |E_(k+1) - model's update of E_k| over 10 iterations: {worst:.3e}")
    assert worst < 1e-12
    assert pose[3].tolist() == [0, 0, 0, 1]
    # the result speaks of the last EVALUATED iteration
    assert res.count == trace[-1]["count"] and res.mean_dist == trace[-1]["sums"][27] / trace[-1]["count"]
    # ... and the model's own loop, libm and all, ends within the same bound of it here
    assert np.abs(pc.expected_loop(name)["pose"] - pose).max() < 1e-6


def test_early_stops(ctx):
    c = pc.case("room_l0")
    few = pc.expected("room_l0")["count"] + 1
    pose, res, trace = run_loop(ctx, "room_l0", max_iterations=5, min_pairs=few)
    assert (res.status, res.iterations, len(trace)) == (binding.W_TOO_FEW_PAIRS, 0, 1)
    assert pose.tobytes() == c["estimate"].tobytes() and trace[0]["status"] == binding.W_TOO_FEW_PAIRS
    assert res.count == few - 1 and trace[0]["sums"].tobytes() == pc.expected("room_l0")["sums"].tobytes()
    # with exactly the pairs of E_0 asked for, the first update is made and the second evaluation (fewer pairs, the
    # model says) stops the loop with the estimate so far
    want = jm.align(max_iterations=5, min_pairs=few - 1, **pc.model_args("room_l0"))
    assert (want["status"], want["iterations"]) == (jm.W_TOO_FEW_PAIRS, 1)
    pose, res, trace = run_loop(ctx, "room_l0", max_iterations=5, min_pairs=few - 1)
    assert (res.status, res.iterations, len(trace)) == (binding.W_TOO_FEW_PAIRS, 1, 2)
    assert [t["status"] for t in trace] == [binding.OK, binding.W_TOO_FEW_PAIRS] and res.count == want["trace"][1]["count"]
    assert np.abs(pose - want["pose"]).max() < 1e-12 and pose[:3].tobytes() == trace[1]["pose"].tobytes()
    # every pixel BEHIND: no pair
    c = pc.case("plane_behind")
    pose, res, trace = run_loop(ctx, "plane_behind", max_iterations=4)
    assert (res.status, res.iterations, res.count, res.mean_dist, len(trace)) == (binding.W_TOO_FEW_PAIRS, 0, 0, 0.0, 1)
    assert pose.tobytes() == c["estimate"].tobytes()
    # a fronto-parallel plane: the normal equations are not positive definite
    c = pc.case("plane")
    pose, res, trace = run_loop(ctx, "plane", max_iterations=4)
    assert (res.status, res.iterations, len(trace)) == (binding.W_DEGENERATE, 0, 1)
    assert pose.tobytes() == c["estimate"].tobytes() and res.count == pc.expected("plane")["count"] == 432


def snapshot(c, levels):
    """what the projective calls must leave alone: the clouds, the associations, the maps, the pyramid, the volume"""
    idx, dist = c.get_associations()
    view = c.tsdf_get_raycast()
    return [c.get_source().tobytes(), c.get_target().tobytes(), c.get_target_normals().tobytes(), idx.tobytes(), dist.tobytes()] + \
        [view[k].tobytes() for k in ("points", "normals", "depth")] + [depth.pyramid_level(c, l).tobytes() for l in range(levels)] + \
        [a.tobytes() for a in c.tsdf_get()[:2]]


def test_the_context_is_left_alone(ctx):
    """After any of the calls the source, target, associations, maps, pyramid and volume are the bytes from before; an
    icpk_align behind them gives what it gives on a context that never made them; two calls in a row give the same
    bytes; and a context that did other work first gives a fresh context's bytes."""
    name = "room_l1"
    c = pc.case(name)
    d3 = tc.case("room")["frames"][2][0]
    kw = dict(solve=binding.SOLVE_POINT_TO_PLANE, max_iterations=4, max_nn_dist=0.1)

    def clouds(x):
        x.backproject_with_normals(d3, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
        x.set_source(synth.backproject(c["depth"], None, tc.ROOM_FX, tc.ROOM_CX))

    with binding.Context(0) as fresh:
        p = pc.device_setup(fresh, name, depth, binding)
        want = [binding.align_projective(fresh, c["estimate"], p), binding.projective_trace(fresh), binding.projective_reduce(fresh, c["estimate"], p),
                binding.projective_associate(fresh, c["estimate"], p)]
    with binding.Context(0) as plain:
        clouds(plain)
        T0, st0, _ = plain.align(**kw)
        assoc0 = plain.get_associations()
    # this context has done other work first: the module's context has run the cases above; now a ray cast at another
    # shape and an alignment
    clouds(ctx)
    ctx.align(**kw)
    pc.device_setup(ctx, "17x19", depth, binding)
    p = pc.device_setup(ctx, name, depth, binding)
    clouds(ctx)
    ctx.nn()
    before = snapshot(ctx, 2)
    got = [binding.align_projective(ctx, c["estimate"], p), binding.projective_trace(ctx), binding.projective_reduce(ctx, c["estimate"], p),
           binding.projective_associate(ctx, c["estimate"], p)]
    again = [binding.align_projective(ctx, c["estimate"], p), binding.projective_trace(ctx), binding.projective_reduce(ctx, c["estimate"], p),
             binding.projective_associate(ctx, c["estimate"], p)]
    assert snapshot(ctx, 2) == before

    def blob(r):
        (pose, res), trace, (sums, count), (pixel, dist) = r
        return [pose.tobytes(), bytes(res), sums.tobytes(), count, pixel.tobytes(), dist.tobytes()] + \
            [t["pose"].tobytes() + t["sums"].tobytes() + bytes([t["status"]]) + str(t["count"]).encode() for t in trace]

    assert blob(got) == blob(want) and blob(again) == blob(want)
    T1, st1, _ = ctx.align(**kw)
    assoc1 = ctx.get_associations()
    assert same_bits(T1, T0) and st1.final_pairs == st0.final_pairs and st1.final_mse == st0.final_mse
    assert same_bits(assoc1[0], assoc0[0]) and same_bits(assoc1[1], assoc0[1])


def test_not_set_and_every_refusal():
    c = pc.case("room_l1")
    E, NS = binding.E_ARG, binding.E_NOT_SET
    P = c["estimate"]
    calls = lambda x: tuple(functools.partial(f, x) for f in (binding.align_projective, binding.projective_reduce, binding.projective_associate))
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
        assert binding.projective_trace(x) == []
        p = pc.device_setup(x, "room_l1", depth, binding)
        good = binding.align_projective(x, P, p)
        trace = binding.projective_trace(x)
        bad = P.copy()
        bad[0, 3] = np.nan
        for call in calls(x):
            assert code_of(call, bad, p) == E
            for kw in (dict(level=2), dict(level=-1), dict(fx=0.0), dict(fx=np.inf), dict(cx=np.nan), dict(max_dist=0.0),
                       dict(max_dist=np.nan), dict(min_pairs=0), dict(max_iterations=0), dict(max_iterations=65)):
                assert code_of(call, P, level=kw.get("level", 1), **{k: v for k, v in kw.items() if k != "level"}) == E, kw
        lib, h = x._lib, x._h
        assert lib.icpk_align_projective(h, C.byref(p), None, None, None) == E
        assert lib.icpk_get_projective_trace(h, None, 4) == E and lib.icpk_get_projective_trace(h, None, 0) == 0
        # a refused call has left everything as it was
        t2 = binding.projective_trace(x)
        assert len(t2) == len(trace) == 10 and all(a["sums"].tobytes() == b["sums"].tobytes() for a, b in zip(t2, trace))
        again = binding.align_projective(x, P, p)
        assert again[0].tobytes() == good[0].tobytes() and bytes(again[1]) == bytes(good[1])
        # NULL outputs are allowed
        assert lib.icpk_align_projective(h, C.byref(p), P.ctypes.data_as(C.POINTER(C.c_double)), None, None) == binding.OK
        x.tsdf_reset()
        for call in calls(x):
            assert code_of(call, P, p) == NS  # the reset volume has no ray cast


# ---- the tracker ------------------------------------------------------------------------------------------------------
def noisy_room_frames():
    """the three frames of the TSDF room case with sensor noise: (depth, true pose)"""
    rng = np.random.default_rng(5)
    out = []
    for rot, shift in tc.ROOM_MOTIONS:
        P = tc.pose(rot, shift)
        out.append((synth.render_room_depth(*tc.ROOM_SHAPE, P[:3, :3], P[:3, 3], tc.ROOM_FX, tc.ROOM_CX, 0.002, rng), P))
    return out


@pytest.mark.parametrize("counts", [(10, 5, 4), None])
def test_model_tracker_projective_is_the_hand_written_loop(ctx, counts):
    frames = noisy_room_frames()
    levels = 1 if counts is None else len(counts)
    iters = (7,) if counts is None else counts
    kw = dict(max_iterations=7) if counts is None else dict(pyramid=counts)
    vol = TsdfVolume(ctx, **GEOM, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
    tracker = ModelTracker(vol, pose=frames[0][1], step=0.125, projective=True, **kw)
    poses = [tracker.track(d) for d, _ in frames]
    planes = vol.planes()
    assert tracker.frames == 3 and tracker.levels_skipped == 0
    assert [st.iterations for st in tracker.level_stats] == list(iters) and all(st.status == binding.OK for st in tracker.level_stats)
    with binding.Context(0) as hand:
        hand.tsdf_create(**GEOM)
        pose, by_hand = frames[0][1].copy(), []
        for k, (d, _) in enumerate(frames):
            if k > 0:
                shapes = depth.build_pyramid(hand, d, depth.pyramid_params(levels=levels))
                estimate = pose
                for l in range(levels - 1, -1, -1):
                    hand.tsdf_raycast(pose, shape=shapes[l], fx=tc.ROOM_FX / 2 ** l, cx=tc.ROOM_CX / 2 ** l, z_near=0.25, z_far=6.0,
                                      step=0.125, min_weight=1)  # the LAST frame's pose at every level
                    estimate, _ = binding.align_projective(hand, estimate, level=l, fx=tc.ROOM_FX, cx=tc.ROOM_CX, max_iterations=iters[l],
                                                        max_dist=0.5)  # the same gate at every level
                pose = estimate
            hand.tsdf_integrate(d, pose, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
            by_hand.append(pose.copy())
        want = hand.tsdf_get()
    assert all(same_bits(a, b) for a, b in zip(poses, by_hand))
    assert not np.array_equal(poses[1], frames[0][1]) and not np.array_equal(poses[2], poses[1])
    assert same_bits(planes[0], want[0]) and same_bits(planes[1], want[1])


def test_projective_none_is_the_tracker_as_it_was(ctx):
    frames = noisy_room_frames()

    def run(**extra):
        vol = TsdfVolume(ctx, **GEOM, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
        t = ModelTracker(vol, pose=frames[0][1], step=0.125, max_nn_dist=0.1, **extra)
        return [t.track(d) for d, _ in frames], vol.planes()[:2], t

    for extra in (dict(max_iterations=12), dict(pyramid=(10, 5, 4))):
        a, pa, ta = run(**extra)
        b, pb, tb = run(projective=None, **extra)
        assert ta.projective is None and tb.projective is None
        assert all(same_bits(x, y) for x, y in zip(a, b)) and all(same_bits(x, y) for x, y in zip(pa, pb))
    # a level without enough hits is skipped and counted; only level 0 raises
    vol = TsdfVolume(ctx, **GEOM, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
    t = ModelTracker(vol, pose=frames[0][1], step=0.125, projective=dict(min_pairs=1500), pyramid=(10, 5, 4))
    t.track(frames[0][0])
    t.track(frames[1][0])
    assert t.levels_skipped == 1 and t.level_stats[2] is None and t.level_hits[2] < 1500 <= t.level_hits[1]
    t2 = ModelTracker(vol, pose=frames[0][1], step=0.125, projective=True, pyramid=(10, 5, 4), min_pairs=30000)
    t2.frames = 1
    with pytest.raises(RuntimeError, match="fewer than min_pairs"):
        t2.track(frames[1][0])
    assert t2.levels_skipped == 2


def test_the_four_room_frames_by_projective_association(ctx):
    """K20's test with projective pairs through max_dist = 0.5, 20 iterations: every frame is placed by its
    predecessor's true pose, the model is built from the tracker's own estimates; the yardstick is the last pair aligned
    frame to frame and the volume's voxel.  The float32 model of tests/projective_model.py over the numpy volume and ray
    cast gave 0.019 deg / 3.83 mm, 0.537 deg / 8.28 mm and 0.165 deg / 7.15 mm after frames 1, 2, 3 before this ran on
    a device."""
    c = tc.case("room")
    d4, P4 = tc.room_frame(*tc.ROOM_FOURTH)
    frames = [(d, P) for d, P, _ in c["frames"]] + [(d4, P4)]
    vol = TsdfVolume(ctx, **GEOM, fx=c["fx"], cx=c["cx"])
    tracker = ModelTracker(vol, pose=frames[0][1], z_near=0.25, z_far=6.0, step=0.125, projective=dict(max_dist=0.5), max_iterations=20)
    errors = []
    for k, (d, P) in enumerate(frames):
        if k > 0:
            tracker.pose = frames[k - 1][1].copy()
        errors.append(pose_error(tracker.track(d), P))
    assert tracker.frames == 4 and tracker.stats.iterations == 20 and errors[0][0] < 1e-9 and errors[0][1] < 1e-12
    P3 = frames[2][1]
    with binding.Context(0) as other:
        other.backproject_with_normals(frames[2][0], fx=c["fx"], cx=c["cx"])
        other.set_source(synth.backproject(d4, None, c["fx"], c["cx"]))
        Tf, _, _ = other.align(solve=binding.SOLVE_POINT_TO_PLANE, max_iterations=20, max_nn_dist=0.1)
    frame_err = pose_error(Tf, np.linalg.inv(P3) @ P4)
    for k, e in enumerate(errors):
        print(f"frame {k}: projective frame-to-model pose error {e[0]:.4f} deg, {1000 * e[1]:.2f} mm")
    print(f"last pair frame to frame: {frame_err[0]:.4f} deg, {1000 * frame_err[1]:.2f} mm")
    assert errors[-1][0] <= frame_err[0]
    assert errors[-1][1] < VOXEL / 2


def test_the_basin_on_the_room(ctx):
    """K24's basin test: the model is the three noiseless room frames fused at their true poses; the next frame is
    rendered at the last pose moved further by s times the motion from it to ROOM_FOURTH, and the trackers start from the
    last true pose.  Projective: 19 iterations through max_dist = 0.5; the unchanged plain tracker: 19 iterations through
    max_nn_dist = 0.1, in the same test.  The bar is K24's separating criterion: within a quarter voxel at s = 1 .. 4, and
    at s = 4 the plain tracker off by more than a voxel."""
    c = tc.case("room")
    (r3, t3), (r4, t4) = tc.ROOM_MOTIONS[2], tc.ROOM_FOURTH
    P3 = tc.pose(r3, t3)
    vol = TsdfVolume(ctx, **GEOM, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
    for d, P, _ in c["frames"]:
        vol.integrate(d, P)
    model = vol.planes()[:2]
    table = []
    for s in (1, 2, 3, 4):
        rot = tuple(a + s * (b - a) for a, b in zip(r3, r4))
        shift = tuple(a + s * (b - a) for a, b in zip(t3, t4))
        d, truth = tc.room_frame(rot, shift)
        row = [s]
        for extra in (dict(max_iterations=19, max_nn_dist=0.1), dict(max_iterations=19, projective=dict(max_dist=0.5))):
            vol.set_planes(*model)
            t = ModelTracker(vol, pose=P3, step=0.125, **extra)
            t.frames = 3  # (the model holds three frames: this one is aligned against it)
            row += pose_error(t.track(d), truth)
        table.append(row)
        print(f"s = {s}: moved {pose_error(P3, truth)[0]:.2f} deg {1000 * pose_error(P3, truth)[1]:.1f} mm; plain "
              f"{row[1]:.4f} deg {1000 * row[2]:.2f} mm; projective {row[3]:.4f} deg {1000 * row[4]:.2f} mm")
    for row in table:
        assert row[4] < VOXEL / 4, row
    assert table[-1][2] > VOXEL, table[-1]
