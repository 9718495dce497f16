"""K29 on the device: icpk_sdf_associate / _reduce against tests/sdf_track_model.py byte for byte on every case of
tests/sdf_track_cases.py; the loop by its trace (the recorded sums are the model's bytes AT the recorded pose, and the next
pose is the model's update of it from those sums); the early stops; what the calls leave alone; a reused context; the
refusals; tsdf.ModelTracker(sdf=...) against the loop written out by hand; and the accuracy tables on the room scene,
printed for DESIGN.md, against K25 and the plain frame-to-frame alignment computed in the same test."""
import ctypes as C
import functools

import numpy as np
import pytest

import projective_model as jm
import sdf_track_cases as sc
import sdf_track_model as sm
import tsdf_cases as tc
from icp_slam_prototype_amd import binding, depth, synth
from icp_slam_prototype_amd.tsdf import ModelTracker, TsdfVolume

pytestmark = pytest.mark.gpu

GEOM = {k: tc.ROOM_VOLUME[k] for k in ("dims", "voxel", "origin", "trunc")}
VOXEL = tc.ROOM_VOLUME["voxel"]
FX, CX = tc.ROOM_FX, tc.ROOM_CX


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
    sc.check_conditions()


@pytest.mark.parametrize("name", sc.NAMES)
def test_associate_and_reduce_give_the_models_bytes(ctx, name):
    c, want = sc.case(name), sc.expected(name)
    p = sc.device_setup(ctx, name, depth, binding)
    # (the inputs the device holds are the model's: the rest compares the rule alone)
    assert same_bits(depth.pyramid_level(ctx, c["level"]), np.array(c["level_image"]))
    f, w, _ = ctx.tsdf_get()
    assert f.tobytes() == c["vol"].tsdf.tobytes() and w.tobytes() == c["vol"].weight.tobytes()
    assert np.array(binding.tsdf_get_params(ctx)[0].origin, np.float32).tobytes() == np.asarray(c["vol"].origin, np.float32).tobytes()
    cell, value = binding.sdf_associate(ctx, c["estimate"], p)
    assert cell.shape == value.shape == c["level_image"].shape
    assert cell.reshape(-1).tobytes() == want["cell"].tobytes()
    assert value.reshape(-1).tobytes() == want["value"].tobytes()
    sums, count = binding.sdf_reduce(ctx, c["estimate"], p)
    assert count == want["count"]
    assert sums.tobytes() == want["sums"].tobytes()


def run_loop(c, name, **kw):
    p = sc.device_setup(c, name, depth, binding)
    for k, v in kw.items():
        setattr(p, k, v)
    pose, res = binding.align_sdf(c, sc.case(name)["estimate"], p)
    return pose, res, binding.sdf_trace(c)


@pytest.mark.parametrize("name", sc.LOOP_CASES)
def test_the_loop_by_its_trace(ctx, name):
    c = sc.case(name)
    pose, res, trace = run_loop(ctx, name, max_iterations=10)
    assert (res.status, res.iterations, len(trace)) == (binding.OK, 10, 10)
    assert trace[0]["pose"].tobytes() == c["estimate"][:3].tobytes()  # E_0 is the input, bit for bit
    worst = 0.0
    for k, it in enumerate(trace):
        assert it["status"] == binding.OK
        E = np.vstack([it["pose"], [0, 0, 0, 1]])
        px = sm.pixels(**sc.model_args(name, pose=E))
        sums, count = sm.reduce(px["terms"], px["cell"])
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


def test_early_stops(ctx):
    c = sc.case("room_l0")
    few = sc.expected("room_l0")["count"] + 1
    pose, res, trace = run_loop(ctx, "room_l0", max_iterations=5, min_pairs=few)
    assert (res.status, res.iterations, len(trace)) == (binding.W_TOO_FEW_PAIRS, 0, 1)
    assert pose.tobytes() == c["estimate"].tobytes() and trace[0]["status"] == binding.W_TOO_FEW_PAIRS
    assert res.count == few - 1 and trace[0]["sums"].tobytes() == sc.expected("room_l0")["sums"].tobytes()
    # no gradient anywhere: no accepted pixel
    c = sc.case("constant")
    pose, res, trace = run_loop(ctx, "constant", max_iterations=4)
    assert (res.status, res.iterations, res.count, res.mean_dist, len(trace)) == (binding.W_TOO_FEW_PAIRS, 0, 0, 0.0, 1)
    assert pose.tobytes() == c["estimate"].tobytes()
    # every point OUTSIDE
    pose, res, trace = run_loop(ctx, "outside", max_iterations=4)
    assert (res.status, res.iterations, res.count, len(trace)) == (binding.W_TOO_FEW_PAIRS, 0, 0, 1)
    # a fronto-parallel plane: the normal equations are not positive definite
    c = sc.case("plane")
    pose, res, trace = run_loop(ctx, "plane", max_iterations=4)
    assert (res.status, res.iterations, len(trace)) == (binding.W_DEGENERATE, 0, 1)
    assert pose.tobytes() == c["estimate"].tobytes() and res.count == sc.expected("plane")["count"]


def sdf_calls(x, P, p):
    """the four calls of the family, as bytes"""
    (pose, res), trace, (sums, count), (cell, value) = binding.align_sdf(x, P, p), binding.sdf_trace(x), \
        binding.sdf_reduce(x, P, p), binding.sdf_associate(x, P, p)
    return [pose.tobytes(), bytes(res), sums.tobytes(), count, cell.tobytes(), value.tobytes()] + \
        [t["pose"].tobytes() + t["sums"].tobytes() + bytes([t["status"]]) + str(t["count"]).encode() for t in trace]


def test_the_state_of_the_context_is_left_untouched():
    """A context that makes sdf calls between a ray cast, a projective alignment, a surface extraction, a mesh extraction
    and a frame-view build returns the same bytes as a context that made none: the same maps, the same projective trace,
    the same list, the same mesh, the same frame view, the same planes and pyramid, the same clouds and associations."""
    t = tc.case("room")
    d4 = sc.case("room_l0")["depth"]
    P3 = sc.P3()
    sp = binding.default_sdf_params(fx=FX, cx=CX, max_iterations=3)

    def run(x, between):
        out = []
        x.tsdf_create(**GEOM)
        for d, P, _ in t["frames"]:
            x.tsdf_integrate(d, P, fx=FX, cx=CX)
        depth.build_pyramid(x, d4, depth.pyramid_params(levels=2))
        x.backproject_with_normals(t["frames"][2][0], fx=FX, cx=CX)
        x.set_source(synth.backproject(d4, None, FX, CX))
        x.nn()
        between(x)
        x.tsdf_raycast(P3, shape=tc.ROOM_SHAPE, fx=FX, cx=CX, z_near=0.25, z_far=6.0, step=0.125, min_weight=1)
        between(x)
        pose, res = binding.align_projective(x, P3, level=0, fx=FX, cx=CX, max_iterations=4)
        out += [pose.tobytes(), bytes(res)]
        between(x)
        x.tsdf_extract_surface(1)
        between(x)
        x.tsdf_extract_mesh(1)
        between(x)
        binding.frame_view_build(x, P3, fx=FX, cx=CX)
        between(x)
        view, surf, mesh = x.tsdf_get_raycast(), x.tsdf_get_surface(), x.tsdf_get_mesh()
        out += [view[k].tobytes() for k in ("points", "normals", "depth")]
        out += [tr["pose"].tobytes() + tr["sums"].tobytes() + str((tr["count"], tr["status"])).encode() for tr in binding.projective_trace(x)]
        out += [surf[k].tobytes() for k in ("points", "normals", "voxel", "axis")]
        out += [mesh[k].tobytes() for k in ("vertices", "normals", "voxel_index", "edge", "triangles")]
        out += [binding.frame_view(x, l).tobytes() for l in (0, 1)]
        out += [a.tobytes() for a in x.tsdf_get()[:2]] + [depth.pyramid_level(x, l).tobytes() for l in (0, 1)]
        idx, dist = x.get_associations()
        out += [x.get_source().tobytes(), x.get_target().tobytes(), x.get_target_normals().tobytes(), idx.tobytes(), dist.tobytes()]
        return out

    made = []
    with binding.Context(0) as quiet:
        want = run(quiet, lambda x: None)
    with binding.Context(0) as busy:
        got = run(busy, lambda x: made.append(sdf_calls(x, P3, sp)))
    assert len(made) == 6 and all(m == made[0] for m in made)  # (and the sdf calls do not see the others either)
    assert len(got) == len(want) and all(a == b for a, b in zip(got, want))


def test_a_reused_context_gives_a_fresh_contexts_bytes(ctx):
    name = "room_l1"
    c = sc.case(name)
    with binding.Context(0) as fresh:
        p = sc.device_setup(fresh, name, depth, binding)
        want = sdf_calls(fresh, c["estimate"], p)
    # the module's context has run the cases above; now another shape, another volume and a stopped loop first
    run_loop(ctx, "260x260", max_iterations=2)
    run_loop(ctx, "constant", max_iterations=3)
    p = sc.device_setup(ctx, name, depth, binding)
    assert sdf_calls(ctx, c["estimate"], p) == want
    assert sdf_calls(ctx, c["estimate"], p) == want  # (and twice in a row)


def test_not_set_and_every_refusal():
    name = "room_l1"
    c = sc.case(name)
    E, NS = binding.E_ARG, binding.E_NOT_SET
    P = c["estimate"]
    calls = lambda x: tuple(functools.partial(f, x) for f in (binding.align_sdf, binding.sdf_reduce, binding.sdf_associate))
    with binding.Context(0) as x:
        for call in calls(x):
            assert code_of(call, P) == NS  # no volume
        x.tsdf_create(**GEOM)
        for call in calls(x):
            assert code_of(call, P) == NS  # no pyramid
        assert binding.sdf_trace(x) == []
        p = sc.device_setup(x, name, depth, binding)
        good = binding.align_sdf(x, P, p)
        trace = binding.sdf_trace(x)
        bad = P.copy()
        bad[0, 3] = np.nan
        for call in calls(x):
            assert code_of(call, bad, p) == E
            for kw in (dict(level=2), dict(level=-1), dict(fx=0.0), dict(fx=np.inf), dict(cx=np.nan), dict(min_pairs=0),
                       dict(max_iterations=0), dict(max_iterations=65), dict(min_normal_cos=np.nan), dict(max_abs_tsdf=0.0),
                       dict(max_abs_tsdf=1.25), dict(max_abs_tsdf=np.nan), dict(min_weight=0), dict(min_weight=65536)):
                assert code_of(call, P, level=kw.get("level", 1), **{k: v for k, v in kw.items() if k != "level"}) == E, kw
        lib, h = x._lib, x._h
        assert lib.icpk_align_sdf(h, C.byref(p), None, None, None) == E
        assert lib.icpk_get_sdf_trace(h, None, 4) == E and lib.icpk_get_sdf_trace(h, None, 0) == 0
        # a refused call has left everything as it was
        t2 = binding.sdf_trace(x)
        assert len(t2) == len(trace) == 10 and all(a["sums"].tobytes() == b["sums"].tobytes() for a, b in zip(t2, trace))
        again = binding.align_sdf(x, P, p)
        assert again[0].tobytes() == good[0].tobytes() and bytes(again[1]) == bytes(good[1])
        # NULL outputs are allowed
        assert lib.icpk_align_sdf(h, C.byref(p), P.ctypes.data_as(C.POINTER(C.c_double)), None, None) == binding.OK
        assert lib.icpk_sdf_associate(h, C.byref(p), P.ctypes.data_as(C.POINTER(C.c_double)), None, None) == binding.OK
        x.tsdf_release()
        for call in calls(x):
            assert code_of(call, P, p) == NS  # the volume is gone


# ---- the tracker ------------------------------------------------------------------------------------------------------
def four_room_frames():
    """the three frames of the TSDF room case with sensor noise and ROOM_FOURTH behind them: (depth, true pose)"""
    rng = np.random.default_rng(5)
    out = []
    for rot, shift in list(tc.ROOM_MOTIONS) + [tc.ROOM_FOURTH]:
        P = tc.pose(rot, shift)
        out.append((synth.render_room_depth(*tc.ROOM_SHAPE, P[:3, :3], P[:3, 3], FX, CX, 0.002, rng), P))
    return out


def drifting_room_frames():
    """four noiseless room frames whose camera drifts 4 cm a frame along x, past a voxel by the third: (depth, true pose)"""
    return [tc.room_frame((0.0, float(k), 0.0), (0.04 * k, 0.01 * (k > 1), 0.01 * (k > 2))) for k in range(4)]


@pytest.mark.parametrize("sdf,counts,follow", [(True, (10, 5, 4), None), (dict(max_abs_tsdf=0.25), None, None),
                                               (dict(max_abs_tsdf=0.25), (10, 5, 4), 1)])
def test_model_tracker_sdf_is_the_hand_written_sequence(ctx, sdf, counts, follow):
    frames = four_room_frames() if follow is None else drifting_room_frames()
    levels = 1 if counts is None else len(counts)
    iters = (7,) if counts is None else counts
    kw = dict(max_iterations=7) if counts is None else dict(pyramid=counts)
    gate = {} if sdf is True else sdf
    vol = TsdfVolume(ctx, **GEOM, fx=FX, cx=CX)
    tracker = ModelTracker(vol, pose=frames[0][1], sdf=sdf, follow=follow, **kw)
    poses = [tracker.track(d) for d, _ in frames]
    planes = vol.planes()
    assert tracker.frames == 4 and tracker.n_hits is None and tracker.level_hits is None and tracker.levels_skipped == 0
    assert [st.iterations for st in tracker.level_stats] == list(iters) and all(st.status == binding.OK for st in tracker.level_stats)
    assert tracker.stats is tracker.level_stats[0]
    assert (tracker.shifts > 0) == (follow is not None)
    with binding.Context(0) as hand:
        hvol = TsdfVolume(hand, **GEOM, fx=FX, cx=CX)
        pose, by_hand = frames[0][1].copy(), []
        for k, (d, _) in enumerate(frames):
            if k > 0:
                depth.build_pyramid(hand, d, depth.pyramid_params(levels=levels))
                for l in range(levels - 1, -1, -1):  # no ray cast at any level
                    pose, _ = binding.align_sdf(hand, pose, level=l, fx=FX, cx=CX, max_iterations=iters[l], **gate)
            if follow is not None:
                hvol.follow(pose, follow)
            hand.tsdf_integrate(d, pose, fx=FX, cx=CX)
            by_hand.append(pose.copy())
        assert code_of(hand.tsdf_get_raycast) == binding.E_NOT_SET  # (nothing was ever cast)
        want = hand.tsdf_get()
    assert code_of(ctx.tsdf_get_raycast) == binding.E_NOT_SET
    assert all(same_bits(a, b) for a, b in zip(poses, by_hand))
    assert not np.array_equal(poses[1], frames[0][1]) and not np.array_equal(poses[2], poses[1])
    assert same_bits(planes[0], want[0]) and same_bits(planes[1], want[1])
    err = pose_error(poses[3], frames[3][1])
    print(f"sdf {sdf}, counts {counts}, follow {follow}: the fourth frame ends {err[0]:.4f} deg, {1000 * err[1]:.2f} mm from its pose")


def test_model_tracker_sdf_settings_and_value_errors(ctx):
    vol = TsdfVolume(ctx, **GEOM, fx=FX, cx=CX)
    for other in (dict(projective=True), dict(projective=True, projective_color=True), dict(projective=True, relocalise=True),
                  dict(projective=dict(max_dist=0.5))):
        with pytest.raises(ValueError, match="sdf does not go together"):
            ModelTracker(vol, sdf=True, **other)
    with pytest.raises(ValueError, match="no setting"):
        ModelTracker(vol, sdf=dict(max_dist=0.5))
    t = ModelTracker(vol, sdf=True, min_pairs=9, min_weight=2)
    assert t.sdf == dict(min_pairs=9) and t.sdf_counts == (10,) and t.projective is None
    plain = ModelTracker(vol, pyramid=(10, 5, 4))
    assert plain.sdf is None


# ---- accuracy -----------------------------------------------------------------------------------------------------------
# tests/sdf_track_model.py over the numpy volume, run on the CPU before anything ran on a device, gave (deg, mm):
#   room pair, default max_abs_tsdf = 1.0: (19,) 0.6071, 37.93; (10, 5, 4) 0.6233, 38.99 -- both bars MISSED: the loop does
#     not settle, its iterates alternate between 27 and 38 mm (DESIGN.md K29 says why); these rows are printed, not held
#     to the bars.
#   room pair, max_abs_tsdf = 0.25 (one voxel of the room volume): (19,) 0.0807, 2.78; (10, 5, 4) 0.0829, 2.89.
#   the basin, s = 1 .. 4, (19,) / (10, 5, 4) / K25's model:
#     default: 0.6071 37.93 / 0.6233 38.99 / 0.4450 4.30;  0.6062 41.91 / 0.6085 41.96 / 0.2534 3.23;
#              0.6585 68.92 / 0.6414 69.28 / 0.3904 4.21;  0.2781 48.05 / 0.3654 57.59 / 0.3170 4.53
#     0.25:    0.0807 2.78 / 0.0829 2.89;  0.0307 5.42 / 0.0335 5.73;  12.40 380.9 / 12.66 528.1 (lost);  19.07 789.6 /
#              19.16 794.5 (lost)
TIGHT = 0.25
TIGHT_HELD_BY_THE_MODEL = (1, 2)  # the s at which the model with max_abs_tsdf = 0.25 ends within half a voxel


def plain_frame_to_frame(target_depth, target_pose, frame_depth, truth, iterations):
    """the project's plain frame-to-frame point-to-plane alignment of the pair: its pose error"""
    with binding.Context(0) as other:
        other.backproject_with_normals(target_depth, fx=FX, cx=CX)
        other.set_source(synth.backproject(frame_depth, None, FX, CX))
        Tf, _, _ = other.align(solve=binding.SOLVE_POINT_TO_PLANE, max_iterations=iterations, max_nn_dist=0.1)
    return pose_error(Tf, np.linalg.inv(target_pose) @ truth)


def sdf_errors(ctx, model, P3, d, truth, cap):
    """(deg, m) of this loop at level 0 with 19 iterations and with (10, 5, 4), and of K25 with 19, on the model volume"""
    row = []
    vol = TsdfVolume(ctx, **GEOM, fx=FX, cx=CX)
    for extra in (dict(max_iterations=19, sdf=dict(max_abs_tsdf=cap)), dict(pyramid=(10, 5, 4), sdf=dict(max_abs_tsdf=cap)),
                  dict(max_iterations=19, step=0.125, projective=dict(max_dist=0.5))):
        vol.set_planes(*model)
        t = ModelTracker(vol, pose=P3, **extra)
        t.frames = 3  # (the model holds three frames: this one is aligned against it)
        row.append(pose_error(t.track(d), truth))
    return row


def fused_room(ctx):
    vol = TsdfVolume(ctx, **GEOM, fx=FX, cx=CX)
    for d, P, _ in tc.case("room")["frames"]:
        vol.integrate(d, P)
    return vol.planes()[:2]


def test_the_room_pair(ctx):
    """The model is fused from the three room frames; ROOM_FOURTH starts at P3.  The bars are K28's: translation error below
    half the room volume's voxel (31.25 mm), rotation error below the plain frame-to-frame alignment's, which is computed
    here with K25's figure beside it.  With the default max_abs_tsdf the numpy model missed both bars before this ran on a
    device, so that row is printed and held only to what the model shows: it ends nearer than it started.  With
    max_abs_tsdf = 0.25 the model met both, and the device is held to them."""
    c = tc.case("room")
    d3, P3 = c["frames"][2][0], c["frames"][2][1]
    d4, truth = tc.room_frame(*tc.ROOM_FOURTH)
    model = fused_room(ctx)
    frame_err = plain_frame_to_frame(d3, P3, d4, truth, 19)
    start = pose_error(P3, truth)
    for cap in (1.0, TIGHT):
        l0, pyr, k25 = sdf_errors(ctx, model, P3, d4, truth, cap)
        print(f"max_abs_tsdf {cap}: sdf (19,) {l0[0]:.4f} deg, {1000 * l0[1]:.2f} mm; sdf (10, 5, 4) {pyr[0]:.4f} deg, "
              f"{1000 * pyr[1]:.2f} mm; K25 {k25[0]:.4f} deg, {1000 * k25[1]:.2f} mm; plain frame to frame {frame_err[0]:.4f} deg, "
              f"{1000 * frame_err[1]:.2f} mm; start {start[0]:.2f} deg, {1000 * start[1]:.1f} mm")
        for e in (l0, pyr):
            assert e[1] < start[1] and e[0] < start[0]
            if cap == TIGHT:
                assert e[1] < VOXEL / 2
                assert e[0] < frame_err[0]


def test_the_basin_on_the_room(ctx):
    """K24's basin: the next frame is rendered at the last pose moved further by s times the motion from it to
    ROOM_FOURTH, and every loop starts from the last true pose.  Three columns: this loop at level 0 (19 iterations), with
    the pyramid (10, 5, 4), and K25 (19 iterations through max_dist = 0.5).  A negative result is a result: with the
    default gate the loop is never lost but never settles either; with max_abs_tsdf = 0.25 it is exact while the start is
    within the gate's reach and lost beyond it."""
    (r3, t3), (r4, t4) = tc.ROOM_MOTIONS[2], tc.ROOM_FOURTH
    P3 = tc.pose(r3, t3)
    model = fused_room(ctx)
    for s in (1, 2, 3, 4):
        rot = tuple(a + s * (b - a) for a, b in zip(r3, r4))
        shift = tuple(a + s * (b - a) for a, b in zip(t3, t4))
        d, truth = tc.room_frame(rot, shift)
        start = pose_error(P3, truth)
        for cap in (1.0, TIGHT):
            l0, pyr, k25 = sdf_errors(ctx, model, P3, d, truth, cap)
            lost = "" if max(l0[1], pyr[1]) < start[1] else "  LOST"
            print(f"s = {s}, max_abs_tsdf {cap}: moved {start[0]:.2f} deg {1000 * start[1]:.1f} mm; sdf (19,) {l0[0]:.4f} deg "
                  f"{1000 * l0[1]:.2f} mm; sdf (10, 5, 4) {pyr[0]:.4f} deg {1000 * pyr[1]:.2f} mm; K25 {k25[0]:.4f} deg "
                  f"{1000 * k25[1]:.2f} mm{lost}")
            if cap == 1.0:  # what the model shows of the default: nearer than the start at every s
                assert l0[1] < start[1] and pyr[1] < start[1], s
            elif s in TIGHT_HELD_BY_THE_MODEL:
                assert l0[1] < VOXEL / 2 and pyr[1] < VOXEL / 2, s
