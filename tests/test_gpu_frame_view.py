"""K28 on the device: icpk_frame_view_build against tests/frame_view_model.py byte for byte on every case of
tests/frame_view_cases.py, and who owns the snapshot; the projective calls through ICPK_VIEW_FRAME against
icpk_projective_pixels fed the same planes, and the loop by its trace; that nothing moved for a context that leaves the
selector alone; the colour gradients and the coloured loop on a frame-view level; odometry.ProjectiveOdometry against
the calls written out by hand, and its keyframe policy; the refusals; and the accuracy on the room against the project's
own frame-to-frame alignment run in the same test, with the tables printed for DESIGN.md."""
import ctypes as C
import functools

import numpy as np
import pytest

import frame_view_cases as fc
import gicp_model
import projective_cases as pc
import projective_color_model as qm
import projective_model as jm
import tsdf_cases as tc
from icp_slam_prototype_amd import binding, depth, synth
from icp_slam_prototype_amd.odometry import ProjectiveOdometry

pytestmark = pytest.mark.gpu

VOXEL = tc.ROOM_VOLUME["voxel"]
FX, CX = tc.ROOM_FX, tc.ROOM_CX


@pytest.fixture(scope="module")
def ctx():
    with binding.Context(0) as c:  # (this context never creates a volume)
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


def build(c, name):
    fc.device_setup(c, name, depth)
    k = fc.case(name)
    return binding.frame_view_build(c, k["pose"], fx=k["fx"], cx=k["cx"])


def check_against_model(c, name, counts):
    k = fc.case(name)
    assert binding.frame_view_levels(c) == k["levels"]
    for l in range(k["levels"]):
        want = fc.expected(name, l)
        assert (counts[0][l], counts[1][l]) == (want["n_valid"], want["n_no_normal"]), (name, l)
        assert binding.frame_view_shape(c, l) == k["images"][l].shape
        assert same_bits(binding.frame_view(c, l), np.array(want["planes"])), (name, l)


# ---- bits and ownership -----------------------------------------------------------------------------------------------
def test_the_cases_hold_their_condition_before_anything_runs():
    fc.check_conditions()


@pytest.mark.parametrize("name", fc.NAMES)
def test_build_gives_the_models_bytes(ctx, name):
    k = fc.case(name)
    counts = build(ctx, name)
    # (the inputs the device holds are the model's: the rest compares the rule alone)
    for l in range(k["levels"]):
        assert same_bits(depth.pyramid_level(ctx, l), np.array(k["images"][l]))
        if k["intensities"] is not None:
            assert same_bits(binding.pyramid_intensity(ctx, l), np.array(k["intensities"][l]))
    check_against_model(ctx, name, counts)
    # a second call, and one that asks for no count (it does not wait), give the same bytes
    check_against_model(ctx, name, binding.frame_view_build(ctx, k["pose"], fx=k["fx"], cx=k["cx"]))
    assert binding.frame_view_build(ctx, k["pose"], fx=k["fx"], cx=k["cx"], counts=False) is None
    check_against_model(ctx, name, counts)
    # ... and so does a second context
    with binding.Context(0) as other:
        check_against_model(other, name, build(other, name))


def test_the_snapshot_is_the_contexts_own(ctx):
    counts = build(ctx, "room_color")
    # a pyramid of a different frame, of a different shape, with and without intensities: the snapshot stays
    f = fc.next_frame()
    depth.build_pyramid(ctx, f["depth"], depth.pyramid_params(levels=3), intensity=f["intensity"])
    check_against_model(ctx, "room_color", counts)
    fc.device_setup(ctx, "5x7_hole", depth)
    check_against_model(ctx, "room_color", counts)
    assert depth.pyramid_shape(ctx, 0) == (5, 7)
    # a rebuild from a one-level pyramid replaces it: levels 1 and 2 are gone
    check_against_model(ctx, "5x7_hole", binding.frame_view_build(ctx, fc.case("5x7_hole")["pose"], fx=16.0, cx=3.0))
    assert code_of(binding.frame_view, ctx, 1) == binding.E_NOT_SET and code_of(binding.frame_view_shape, ctx, 2) == binding.E_NOT_SET
    # release drops it, twice is fine, and a build brings it back
    binding.frame_view_release(ctx)
    binding.frame_view_release(ctx)
    assert binding.frame_view_levels(ctx) == 0 and code_of(binding.frame_view, ctx, 0) == binding.E_NOT_SET
    check_against_model(ctx, "room", build(ctx, "room"))
    # TSDF calls on the same context leave it alone too
    with binding.Context(0) as x:
        counts = build(x, "room")
        x.tsdf_create(**{k: tc.ROOM_VOLUME[k] for k in ("dims", "voxel", "origin", "trunc")})
        for d, P, _ in tc.case("room")["frames"]:
            x.tsdf_integrate(d, P, fx=FX, cx=CX)
        x.tsdf_raycast(fc.case("room")["pose"], **pc.case("room_l0")["view"])
        x.tsdf_reset()
        check_against_model(x, "room", counts)
        x.tsdf_release()
        check_against_model(x, "room", counts)


# ---- the loop through the frame view ---------------------------------------------------------------------------------
def frame_setup(c, level, color=False):
    """the view of frame 3 built, then the fourth frame's pyramid; the selector on the view's level `level`"""
    name = "room_color" if color else "room"
    build(c, name)
    f = fc.next_frame()
    depth.build_pyramid(c, f["depth"], depth.pyramid_params(levels=3), intensity=f["intensity"] if color else None)
    binding.projective_set_view(c, binding.VIEW_FRAME, level)
    return binding.default_projective_params(level=level, fx=FX, cx=CX)


@pytest.fixture
def framed(ctx):
    yield ctx
    binding.projective_set_view(ctx, binding.VIEW_RAYCAST)


@pytest.mark.parametrize("level,gate", [(0, -2.0), (1, -2.0), (2, 0.9)])
def test_associate_and_reduce_are_the_host_rule_on_the_same_planes(framed, level, gate):
    c = framed
    p = frame_setup(c, level)
    p.min_normal_cos = gate
    a = fc.loop_args(level)
    planes = binding.frame_view(c, level)
    assert same_bits(planes, np.array(a["view"]))
    E = tc.pose((2.5, -3.5, 0.3), (-0.04, 0.03, 0.02))  # (neither the view's pose nor the frame's)
    pixel_h, dist_h, terms_h, pairs = binding.projective_pixels(p, E, a["level"], planes, planes.shape[1:], float(a["fx_v"]),
                                                               float(a["cx_v"]), a["view_pose"], terms=True)
    pixel, dist = binding.projective_associate(c, E, p)
    assert pixel.reshape(-1).tobytes() == pixel_h.tobytes() and dist.reshape(-1).tobytes() == dist_h.tobytes()
    assert 6 < pairs < pixel.size
    sums, count = binding.projective_reduce(c, E, p)
    assert count == pairs and sums.tobytes() == gicp_model.canonical(terms_h).tobytes()
    # through the view's own pose, the view's own frame pairs every listed pixel with itself at distance exactly 0
    depth.build_pyramid(c, fc.case("room")["depth"], depth.pyramid_params(levels=3))
    pixel, dist = binding.projective_associate(c, a["view_pose"], p)
    listed = fc.expected("room", level)["listed"]
    assert np.array_equal(pixel[listed], np.nonzero(listed.reshape(-1))[0]) and not dist.any()
    assert (pixel[~listed] < 0).all()


def check_trace(name, pose, res, trace, model_at, start):
    """test_gpu_projective.py's test_the_loop_by_its_trace, its bars unchanged"""
    assert (res.status, res.iterations, len(trace)) == (binding.OK, 10, 10)
    assert trace[0]["pose"].tobytes() == start[:3].tobytes()  # E_0 is the input, bit for bit
    worst = 0.0
    for k, it in enumerate(trace):
        assert it["status"] == binding.OK
        E = np.vstack([it["pose"], [0, 0, 0, 1]])
        sums, count = model_at(E)
        assert it["count"] == count, k
        assert it["sums"].tobytes() == sums.tobytes(), k  # the model's bytes AT the recorded pose
        status, En = jm.update(it["sums"], it["count"], E)
        nxt = trace[k + 1]["pose"] if k + 1 < len(trace) else pose[:3]
        assert status == jm.OK
        worst = max(worst, float(np.abs(En[:3] - nxt).max()))
    print(f"{name}: largest |E_(k+1) - model's update of E_k| over 10 iterations: {worst:.3e}")
    assert worst < 1e-12
    assert pose[3].tolist() == [0, 0, 0, 1]
    assert res.count == trace[-1]["count"] and res.mean_dist == trace[-1]["sums"][27] / trace[-1]["count"]


@pytest.mark.parametrize("level", [0, 1])
def test_the_loop_by_its_trace(framed, level):
    c = framed
    p = frame_setup(c, level)
    p.max_iterations = 10
    start = fc.case("room")["pose"]
    pose, res = binding.align_projective(c, start, p)

    def model_at(E):
        px = jm.pixels(**fc.loop_args(level, pose=E))
        return jm.reduce(px["terms"], px["pixel"])

    check_trace(f"frame view, level {level}", pose, res, binding.projective_trace(c), model_at, start)
    # ... and the model's own loop, libm and all, ends within the same bound of it here
    assert np.abs(jm.align(max_iterations=10, **fc.loop_args(level))["pose"] - pose).max() < 1e-6
    assert pose_error(pose, fc.next_frame()["truth"])[1] < pose_error(start, fc.next_frame()["truth"])[1]


# ---- nothing moved ----------------------------------------------------------------------------------------------------
def test_with_the_selector_at_its_default_nothing_has_moved():
    """align_projective / align_projective_colored and their traces against a ray cast of the room volume: a context
    that has built a frame view (and its gradients) but left the selector alone gives the bytes of one that never built
    it; one that switched to the frame view and back gives them again."""
    import projective_color_cases as kc
    name = "room_l1"
    c = kc.case(name)

    def run(x):
        geo = binding.align_projective(x, c["estimate"], p)
        tg = binding.projective_trace(x)
        col = binding.align_projective_colored(x, c["estimate"], p)
        tcol = binding.projective_trace(x)
        red = binding.projective_reduce(x, c["estimate"], p)
        pix = binding.projective_associate(x, c["estimate"], p)
        return [geo[0].tobytes(), bytes(geo[1]), col[0].tobytes(), bytes(col[1]), red[0].tobytes(), red[1], pix[0].tobytes(),
                pix[1].tobytes()] + [t["pose"].tobytes() + t["sums"].tobytes() + bytes([t["status"]]) + str(t["count"]).encode()
                                     for t in tg + tcol]

    with binding.Context(0) as plain:
        p = kc.device_setup(plain, name, depth, binding)
        want = run(plain)
    with binding.Context(0) as x:
        p = kc.device_setup(x, name, depth, binding)
        level_pyramid = [depth.pyramid_level(x, l) for l in range(c["level"] + 1)]
        binding.frame_view_build(x, fc.case("room")["pose"], fx=FX, cx=CX)
        for l in range(binding.frame_view_levels(x)):
            binding.frame_view_color_gradients(x, l, fc.GRADIENT_RADIUS * 2 ** l)
        assert run(x) == want
        binding.projective_set_view(x, binding.VIEW_FRAME, 1)
        moved = run(x)
        assert moved != want
        binding.projective_set_view(x, binding.VIEW_RAYCAST, 5)  # (view_level says nothing about a ray cast)
        assert run(x) == want
        # and the frame-view calls have left the pyramid and the ray cast where they were
        assert all(same_bits(depth.pyramid_level(x, l), level_pyramid[l]) for l in range(c["level"] + 1))
        view = x.tsdf_get_raycast()
        assert np.concatenate([view["points"], view["normals"], view["depth"][None]]).tobytes() == kc.maps_of(name)[:7].tobytes()


# ---- colour -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 1, 2])
def test_gradients_on_a_level_are_the_view_gradient_rules_bytes(ctx, level):
    build(ctx, "room_color")
    assert code_of(binding.frame_view_get_color_gradients, ctx, level) == binding.E_NOT_SET
    binding.frame_view_color_gradients(ctx, level, fc.GRADIENT_RADIUS * 2 ** level)
    planes = binding.frame_view(ctx, level)
    got = binding.frame_view_get_color_gradients(ctx, level)
    assert same_bits(got, np.array(fc.view_gradients(level))) and got.any()
    assert same_bits(got, qm.view_gradients(planes, fc.GRADIENT_RADIUS * 2 ** level)[0])
    # the planes are untouched, the other levels have none, and the next build drops them
    assert same_bits(binding.frame_view(ctx, level), planes)
    assert code_of(binding.frame_view_get_color_gradients, ctx, (level + 1) % 3) == binding.E_NOT_SET
    binding.frame_view_build(ctx, fc.case("room_color")["pose"], fx=FX, cx=CX, counts=False)
    assert code_of(binding.frame_view_get_color_gradients, ctx, level) == binding.E_NOT_SET


@pytest.mark.parametrize("level", [0, 1])
def test_the_colored_loop_by_its_trace(framed, level):
    c = framed
    p = frame_setup(c, level, color=True)
    p.max_iterations = 10
    binding.frame_view_color_gradients(c, level, fc.GRADIENT_RADIUS * 2 ** level)
    start = fc.case("room_color")["pose"]
    # lambda_geometric = 1 is the geometric loop bit for bit
    geo, rg = binding.align_projective(c, start, p)
    tg = binding.projective_trace(c)
    one, r1 = binding.align_projective_colored(c, start, p, dict(lambda_geometric=1.0))
    t1 = binding.projective_trace(c)
    assert one.tobytes() == geo.tobytes() and bytes(r1) == bytes(rg)
    assert all(a["pose"].tobytes() == b["pose"].tobytes() and a["sums"].tobytes() == b["sums"].tobytes() for a, b in zip(t1, tg))
    s1 = binding.projective_reduce_colored(c, start, p, dict(lambda_geometric=1.0))
    s0 = binding.projective_reduce(c, start, p)
    assert s1[0].tobytes() == s0[0].tobytes() and s1[1] == s0[1]
    pose, res = binding.align_projective_colored(c, start, p)

    def model_at(E):
        px = qm.pixels(**fc.loop_args(level, pose=E, color=True))
        return qm.reduce(px["terms"], px["pixel"])

    check_trace(f"frame view, coloured, level {level}", pose, res, binding.projective_trace(c), model_at, start)
    assert pose.tobytes() != geo.tobytes()  # the coloured loop is not the geometric one


# ---- the tracker ------------------------------------------------------------------------------------------------------
def noisy_room_frames():
    """the three frames of the TSDF room case and the fourth with sensor noise: (depth, intensity, true pose)"""
    rng = np.random.default_rng(5)
    out = []
    for rot, shift in list(tc.ROOM_MOTIONS) + [tc.ROOM_FOURTH]:
        P = tc.pose(rot, shift)
        out.append((synth.render_room_depth(*tc.ROOM_SHAPE, P[:3, :3], P[:3, 3], FX, CX, 0.002, rng), tc.room_intensity(rot, shift), P))
    return out


@pytest.mark.parametrize("color", [False, True])
def test_projective_odometry_is_the_hand_written_sequence(ctx, color):
    frames = noisy_room_frames()
    counts = (10, 5, 4)
    odo = ProjectiveOdometry(ctx, pose=frames[0][2], pyramid=counts, color=True if color else None, fx=FX, cx=CX)
    poses = [odo.track(d, I if color else None) for d, I, _ in frames]
    assert (odo.frames, odo.views_built, odo.levels_skipped) == (4, 4, 0)
    assert [st.iterations for st in odo.level_stats] == list(counts) and all(st.status == binding.OK for st in odo.level_stats)
    with binding.Context(0) as hand:
        pose, by_hand = frames[0][2].copy(), []
        for k, (d, I, _) in enumerate(frames):
            depth.build_pyramid(hand, d, depth.pyramid_params(levels=3), intensity=I if color else None)
            if k > 0:
                estimate = pose
                for l in (2, 1, 0):
                    binding.projective_set_view(hand, binding.VIEW_FRAME, l)
                    kw = dict(level=l, fx=FX, cx=CX, max_iterations=counts[l], max_dist=0.5)
                    if color:
                        estimate, _ = binding.align_projective_colored(hand, estimate, binding.default_projective_params(**kw))
                    else:
                        estimate, _ = binding.align_projective(hand, estimate, **kw)
                pose = estimate
            binding.frame_view_build(hand, pose, fx=FX, cx=CX, counts=False)
            if color:
                for l in range(3):
                    binding.frame_view_color_gradients(hand, l, 0.1 * 2 ** l, 4)
            by_hand.append(pose.copy())
    assert all(same_bits(a, b) for a, b in zip(poses, by_hand))
    assert not np.array_equal(poses[1], poses[0]) and not np.array_equal(poses[3], poses[2])
    for k in (1, 2, 3):
        e = pose_error(poses[k], frames[k][2])
        print(f"frame {k} ({'coloured' if color else 'geometric'}): frame-to-frame odometry error {e[0]:.4f} deg, {1000 * e[1]:.2f} mm")
    # the selector is back at its default: without a volume the projective calls say so
    assert code_of(binding.align_projective, ctx, poses[0]) == binding.E_NOT_SET


def test_the_keyframe_policy_keeps_the_view_until_a_bound_is_passed(ctx):
    frames = noisy_room_frames()
    moves = [pose_error(frames[k][2], frames[0][2]) for k in range(4)]  # 0, 4, ~4.5, ~2.2 degrees from the first frame
    assert moves[1][0] < 5 and moves[2][0] < 5
    # a bound nothing passes: one view for the whole sequence
    odo = ProjectiveOdometry(ctx, pose=frames[0][2], keyframe=dict(max_angle_deg=30.0, max_shift=1.0, min_overlap=0.1), fx=FX, cx=CX)
    kept = [odo.track(d) for d, _, _ in frames]
    assert odo.views_built == 1 and same_bits(odo.view_pose, frames[0][2])
    # a bound the second frame passes (4 degrees > 3): rebuilt there, and every frame after is measured from the new view
    odo = ProjectiveOdometry(ctx, pose=frames[0][2], keyframe=dict(max_angle_deg=3.0), fx=FX, cx=CX)
    built = []
    for d, _, _ in frames:
        odo.track(d)
        built.append(odo.views_built)
    assert built[:2] == [1, 2] and built[-1] > built[0] and same_bits(odo.view_pose, odo.pose) == (built[3] > built[2])
    # an overlap no frame reaches: rebuilt every frame, which is keyframe=None bit for bit
    every = ProjectiveOdometry(ctx, pose=frames[0][2], keyframe=dict(min_overlap=2.0), fx=FX, cx=CX)
    plain = ProjectiveOdometry(ctx, pose=frames[0][2], fx=FX, cx=CX)
    # (one after the other: a context holds ONE view)
    assert all(same_bits(a, b) for a, b in zip([every.track(d) for d, _, _ in frames], [plain.track(d) for d, _, _ in frames]))
    assert every.views_built == plain.views_built == 4
    # frame to keyframe does not accumulate: the kept view's last pose is as good as the chained one
    print("kept view:", [pose_error(kept[k], frames[k][2]) for k in range(4)])
    # a level without enough valid pixels is skipped and counted; only level 0 raises
    odo = ProjectiveOdometry(ctx, pose=frames[0][2], projective=dict(min_pairs=1500), fx=FX, cx=CX)
    odo.track(frames[0][0])
    odo.track(frames[1][0])
    assert odo.levels_skipped == 1 and odo.level_stats[2] is None and odo.level_valid[2] < 1500 <= odo.level_valid[1]
    odo = ProjectiveOdometry(ctx, pose=frames[0][2], projective=dict(min_pairs=30000), fx=FX, cx=CX)
    odo.track(frames[0][0])
    with pytest.raises(RuntimeError, match="fewer than min_pairs"):
        odo.track(frames[1][0])
    assert odo.levels_skipped == 2
    with pytest.raises(ValueError):
        ProjectiveOdometry(ctx, color=True).track(frames[0][0])


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_not_set_and_every_refusal():
    E, NS = binding.E_ARG, binding.E_NOT_SET
    k = fc.case("room_color")
    P = k["pose"]
    projective = (binding.align_projective, binding.projective_reduce, binding.projective_associate)
    colored = (binding.align_projective_colored, binding.projective_reduce_colored)
    with binding.Context(0) as x:
        assert code_of(binding.frame_view_build, x, P) == NS  # no pyramid
        for call, arg in ((functools.partial(binding.frame_view, x), 0), (functools.partial(binding.frame_view_shape, x), 0), (functools.partial(binding.frame_view_get_color_gradients, x), 0)):
            assert code_of(call, arg) == NS  # no snapshot
        assert code_of(binding.frame_view_color_gradients, x, 0, 0.1) == NS and code_of(binding.projective_set_view, x, binding.VIEW_FRAME, 0) == NS
        assert binding.frame_view_levels(x) == 0
        binding.frame_view_release(x)  # (nothing to drop)
        depth.build_pyramid(x, k["depth"], depth.pyramid_params(levels=2))  # no intensities yet
        bad = P.copy()
        bad[1, 2] = np.inf
        for kw in (dict(pose=bad), dict(pose=None), dict(pose=P, fx=0.0), dict(pose=P, fx=-2.0), dict(pose=P, fx=np.nan),
                   dict(pose=P, fx=np.inf), dict(pose=P, cx=np.nan), dict(pose=P, cx=-np.inf)):
            assert code_of(binding.frame_view_build, x, **kw) == E, kw
        assert binding.frame_view_levels(x) == 0  # a refused call has left everything as it was
        binding.frame_view_build(x, P, fx=FX, cx=CX)
        good = [binding.frame_view(x, l) for l in range(2)]
        for level in (-1, binding.PYRAMID_MAX_LEVELS):
            assert code_of(binding.frame_view, x, level) == E and code_of(binding.projective_set_view, x, binding.VIEW_FRAME, level) == E
        assert code_of(binding.frame_view, x, 2) == NS and code_of(binding.projective_set_view, x, binding.VIEW_FRAME, 2) == NS  # a level it lacks
        for which in (-1, 2):
            assert code_of(binding.projective_set_view, x, which, 0) == E
        assert code_of(binding.frame_view_build, x, bad) == E
        assert all(same_bits(binding.frame_view(x, l), good[l]) for l in range(2))
        # the view was built without intensities: no gradients, no coloured call
        assert code_of(binding.frame_view_color_gradients, x, 0, 0.1) == NS
        binding.projective_set_view(x, binding.VIEW_FRAME, 1)
        for call in projective:
            call(x, P, level=1, fx=FX, cx=CX)  # no volume anywhere: the calls run
        for call in colored:
            assert code_of(call, x, P, level=1, fx=FX, cx=CX) == NS
        # with intensities in the view but none beside the pyramid, and then without gradients of the level
        depth.build_pyramid(x, k["depth"], depth.pyramid_params(levels=2), intensity=k["intensity"])
        binding.frame_view_build(x, P, fx=FX, cx=CX)
        for r in (0.0, -1.0, np.nan, np.inf):
            assert code_of(binding.frame_view_color_gradients, x, 0, r) == E
        assert code_of(binding.frame_view_color_gradients, x, 0, 0.1, 0) == E
        assert x._lib.icpk_frame_view_color_gradients(x._h, 0, 0.1, 4, 1) == E  # flags must be 0
        binding.frame_view_color_gradients(x, 0, 0.1)
        for call in colored:
            assert code_of(call, x, P, level=1, fx=FX, cx=CX) == NS  # level 1 has no gradients
        binding.frame_view_color_gradients(x, 1, 0.2)
        depth.build_pyramid(x, k["depth"], depth.pyramid_params(levels=2))
        for call in colored:
            assert code_of(call, x, P, level=1, fx=FX, cx=CX) == NS  # no intensity pyramid
        depth.build_pyramid(x, k["depth"], depth.pyramid_params(levels=2), intensity=k["intensity"])
        for call in colored:
            call(x, P, level=1, fx=FX, cx=CX)
        # the projective calls' own refusals are unchanged under the frame view
        for call in projective + colored:
            assert code_of(call, x, bad, level=1, fx=FX, cx=CX) == E
            assert code_of(call, x, P, level=2, fx=FX, cx=CX) == E  # a level the PYRAMID lacks
        # without a pyramid the frame-view calls say NOT_SET; after a release so do the projective ones
        binding.frame_view_release(x)
        for call in projective + colored:
            assert code_of(call, x, P, level=1, fx=FX, cx=CX) == NS
        assert code_of(binding.projective_set_view, x, binding.VIEW_FRAME, 0) == NS
        binding.projective_set_view(x, binding.VIEW_RAYCAST)
        for call in projective:
            assert code_of(call, x, P, level=1, fx=FX, cx=CX) == NS  # no volume
        lib, h = x._lib, x._h
        assert lib.icpk_frame_view_get(h, 0, None) == E and lib.icpk_frame_view_build(None, 1.0, 0.0, None, None, None) == E
        assert lib.icpk_frame_view_release(None) == E and lib.icpk_projective_set_view(None, 0, 0) == E
        # NULL planes are allowed
        binding.frame_view_build(x, P, fx=FX, cx=CX, counts=False)
        assert lib.icpk_frame_view_get(h, 0, (C.POINTER(C.c_float) * 8)()) == binding.OK
        assert lib.icpk_frame_view_shape(h, 0, None, None) == binding.OK


# ---- accuracy -----------------------------------------------------------------------------------------------------------
def plain_frame_to_frame(target_depth, target_pose, frame_depth, truth, iterations):
    """the project's plain frame-to-frame point-to-plane alignment of the pair: its pose error"""
    with binding.Context(0) as other:
        other.backproject_with_normals(target_depth, fx=FX, cx=CX)
        other.set_source(synth.backproject(frame_depth, None, FX, CX))
        Tf, _, _ = other.align(solve=binding.SOLVE_POINT_TO_PLANE, max_iterations=iterations, max_nn_dist=0.1)
    return pose_error(Tf, np.linalg.inv(target_pose) @ truth)


def test_the_room_pair_against_the_plain_frame_to_frame_alignment(ctx):
    """Frame 3 to ROOM_FOURTH.  The yardstick is test_the_four_room_frames_by_projective_association's frame_err, computed
    here the same way: the frame-view pose error in rotation is at most that alignment's, and its translation error is
    below half the room volume's voxel."""
    c = tc.case("room")
    d3, P3 = c["frames"][2][0], c["frames"][2][1]
    f = fc.next_frame()
    frame_err = plain_frame_to_frame(d3, P3, f["depth"], f["truth"], 20)
    odo = ProjectiveOdometry(ctx, pose=P3, pyramid=(20,), fx=FX, cx=CX)
    odo.track(d3)
    err = pose_error(odo.track(f["depth"]), f["truth"])
    pyr = ProjectiveOdometry(ctx, pose=P3, fx=FX, cx=CX)
    pyr.track(d3)
    err_pyr = pose_error(pyr.track(f["depth"]), f["truth"])
    print(f"frame view, 20 iterations at level 0: {err[0]:.4f} deg, {1000 * err[1]:.2f} mm; pyramid (10, 5, 4): "
          f"{err_pyr[0]:.4f} deg, {1000 * err_pyr[1]:.2f} mm; plain frame to frame: {frame_err[0]:.4f} deg, {1000 * frame_err[1]:.2f} mm")
    assert odo.level_stats[0].iterations == 20
    assert err[0] <= frame_err[0]
    assert err[1] < VOXEL / 2


# the s of test_the_basin_on_the_room at which the loop's numpy model (tests/projective_model.py over
# tests/frame_view_model.py, 19 iterations at level 0, run on the CPU before this ran on a device) is no worse than the
# plain alignment in both rotation and translation; the whole table is in DESIGN.md, K28
BASIN_HELD_BY_THE_MODEL = (2, 3)


def test_the_basin_on_the_room(ctx):
    """test_gpu_projective.py's basin with the view built from frame 3 ALONE: the next frame is rendered at the last pose
    moved further by s times the motion from it to ROOM_FOURTH; both start from the last true pose.  Frame view: 19
    iterations at level 0 through max_dist = 0.5; the plain frame-to-frame alignment: 19 iterations through
    max_nn_dist = 0.1, in the same test."""
    c = tc.case("room")
    (r3, t3), (r4, t4) = tc.ROOM_MOTIONS[2], tc.ROOM_FOURTH
    d3, P3 = c["frames"][2][0], tc.pose(r3, t3)
    table = []
    for s in (1, 2, 3, 4):
        rot = tuple(a + s * (b - a) for a, b in zip(r3, r4))
        shift = tuple(a + s * (b - a) for a, b in zip(t3, t4))
        d, truth = tc.room_frame(rot, shift)
        plain = plain_frame_to_frame(d3, P3, d, truth, 19)
        row = [s, *plain]
        for counts in ((19,), (10, 5, 4)):
            odo = ProjectiveOdometry(ctx, pose=P3, pyramid=counts, fx=FX, cx=CX)
            odo.track(d3)
            row += pose_error(odo.track(d), truth)
        row.append(odo.level_stats[0].count)
        table.append(row)
        print(f"s = {s}: moved {pose_error(P3, truth)[0]:.2f} deg {1000 * pose_error(P3, truth)[1]:.1f} mm; plain frame to frame "
              f"{row[1]:.4f} deg {1000 * row[2]:.2f} mm; frame view (19,) {row[3]:.4f} deg {1000 * row[4]:.2f} mm; frame view "
              f"(10, 5, 4) {row[5]:.4f} deg {1000 * row[6]:.2f} mm")
    for row in table:
        if row[0] in BASIN_HELD_BY_THE_MODEL:
            assert row[3] <= row[1] and row[4] <= row[2], row
