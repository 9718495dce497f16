"""Signed updates of the TSDF volume on the device (K30; icpk_tsdf_apply, icpk_tsdf_deintegrate) against
tests/tsdf_apply_model.py, bit for bit unless said otherwise: the planes and the per-op counts on every case of
tests/tsdf_apply_cases.py and on a shifted volume, the exact properties of the rule, the derived bound of a removal, every
refusal, what the call leaves alone, and a reused context against a fresh one."""
import numpy as np
import pytest

import tsdf_apply_cases as ac
import tsdf_apply_model as am
import tsdf_cases as tc
import tsdf_model
from icp_slam_prototype_amd import binding, depth as depth_front
from icp_slam_prototype_amd.tsdf import TsdfVolume

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with binding.Context(0) as c:
        yield c


def create(ctx, c, **over):
    v = dict(c["volume"], **over)
    return ctx.tsdf_create(dims=v["dims"], voxel=v["voxel"], origin=v["origin"], trunc=v["trunc"],
                           max_weight=v.get("max_weight"), flags=binding.TSDF_COLOR if v.get("color") else 0)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def planes(ctx, c):
    return ctx.tsdf_get(intensity=bool(c["volume"].get("color")))


def run(ctx, c, ops=None):
    return binding.tsdf_apply(ctx, c["frames"], c["ops"] if ops is None else ops, c["intensities"], fx=c["fx"], cx=c["cx"])


def same_planes(a, b):
    return all((x is None and y is None) or same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ac.BYTE_CASES)
def test_planes_and_counts_match_the_model(ctx, name):
    c, m = ac.case(name), ac.model(name)
    create(ctx, c)
    counts = run(ctx, c)
    assert counts.tolist() == m["counts"]
    f, w, ci = planes(ctx, c)
    assert same_bits(f, m["tsdf"]) and same_bits(w, m["weight"])
    if ci is not None:
        assert same_bits(ci, m["intensity"]) and ci.max() > 0
    if name == "fresh_minus":
        assert counts.tolist() == [0, 0, 0] and f.tobytes() == bytes(f.nbytes) and not w.any()


@pytest.mark.parametrize("name", ["tail", "room_color", "saturation"])
def test_one_call_of_n_ops_is_n_calls_of_one_op(ctx, name):
    c, m = ac.case(name), ac.model(name)
    create(ctx, c)
    counts = []
    for sign, frame, pose in c["ops"]:  # (a call of one op carries one frame)
        img = None if c["intensities"] is None else [c["intensities"][frame]]
        counts.append(int(binding.tsdf_apply(ctx, [c["frames"][frame]], [(sign, 0, pose)], img, fx=c["fx"], cx=c["cx"])[0]))
    assert counts == m["counts"]
    f, w, ci = planes(ctx, c)
    assert same_bits(f, m["tsdf"]) and same_bits(w, m["weight"]) and (ci is None or same_bits(ci, m["intensity"]))


@pytest.mark.parametrize("name", ["room_color", "odd", "saturation"])
def test_a_single_plus_op_is_integrate(ctx, name):
    c = tc.case(name)
    color = bool(c["volume"].get("color"))
    create(ctx, c)
    want_n = [ctx.tsdf_integrate(d, P, img, fx=c["fx"], cx=c["cx"]) for d, P, img in c["frames"]]
    want = ctx.tsdf_get(intensity=color)
    ctx.tsdf_reset()
    got_n = [int(binding.tsdf_apply(ctx, [d], [(+1, 0, P)], None if img is None else [img], fx=c["fx"], cx=c["cx"])[0])
             for d, P, img in c["frames"]]
    assert got_n == want_n and same_planes(ctx.tsdf_get(intensity=color), want)


def test_plus_then_minus_on_a_fresh_volume_gives_the_fresh_bytes(ctx):
    c = tc.case("room_color")
    create(ctx, c)
    d, P, img = c["frames"][1]
    n = binding.tsdf_apply(ctx, [d], [(+1, 0, P), (-1, 0, P)], [img], fx=c["fx"], cx=c["cx"])
    assert n[0] == n[1] > 0
    for a in ctx.tsdf_get(intensity=True):
        assert a.tobytes() == bytes(a.nbytes)
    # the same through integrate and deintegrate, one call each
    vol = TsdfVolume(ctx, color=True, fx=c["fx"], cx=c["cx"], **{k: c["volume"][k] for k in ("dims", "voxel", "origin", "trunc")})
    assert vol.integrate(d, P, img) == vol.deintegrate(d, P, img) == n[0] and vol.frames == 0
    for a in vol.planes(intensity=True):
        assert a.tobytes() == bytes(a.nbytes)


def test_removal_stays_within_the_derived_bound(ctx):
    """+A +B +C then -B against +A +C, both on the device: the weight planes are equal and the tsdf planes within
    tsdf_apply_cases.REMOVAL_BOUND = 13.5 EPS (1 + 2^-16) = 8.05e-7, the bound derived in tsdf_apply_model.error_bound
    (tests/test_tsdf_apply_host.py confirms it on the model: 1.19e-7 there).  The device gives the model's bytes on both
    sides, so the figure is the model's."""
    a, b = ac.case("abcb"), ac.case("ac")
    create(ctx, a)
    run(ctx, a)
    fa, wa, _ = planes(ctx, a)
    create(ctx, b)
    run(ctx, b)
    fb, wb, _ = planes(ctx, b)
    assert same_bits(wa, wb) and (wa == 2).sum() > 1000
    diff = np.abs(fa.astype(np.float64) - fb.astype(np.float64)).max()
    print(f"removal on the device: max |diff| {diff:.3g}, bound {ac.REMOVAL_BOUND:.3g}")
    assert diff <= ac.REMOVAL_BOUND


def test_a_shifted_volume_takes_the_ops_at_its_current_origin(ctx):
    c = ac.case("room_color")
    create(ctx, c)
    d0, d1 = c["frames"]
    i0, i1 = c["intensities"]
    p0, p1 = c["ops"][1][2], c["ops"][2][2]
    run(ctx, c, [(+1, 0, p0), (+1, 1, p1)])
    binding.tsdf_shift(ctx, (3, -2, 5))
    f, w, ci = ctx.tsdf_get(intensity=True)
    p, total = binding.tsdf_get_params(ctx)
    assert total.tolist() == [3, -2, 5]
    vol = tsdf_model.Volume(**dict(c["volume"], origin=tuple(p.origin)))
    vol.tsdf, vol.weight, vol.intensity = f.copy(), w.copy(), ci.copy()
    ops = [(-1, 0, p0), (+1, 1, ac.drift(p1, (1.0, 0.0, 0.0), (0.02, 0.0, 0.0))), (-1, 1, p1), (+1, 0, p0)]
    want = am.apply(vol, [d0, d1], ops, c["fx"], c["cx"], [i0, i1])
    got = run(ctx, c, ops)
    assert got.tolist() == want and min(want) > 1000
    f, w, ci = ctx.tsdf_get(intensity=True)
    assert same_bits(f, vol.tsdf) and same_bits(w, vol.weight) and same_bits(ci, vol.intensity)
    assert binding.tsdf_get_params(ctx)[1].tolist() == [3, -2, 5]


def test_every_refusal_leaves_the_planes_unchanged(ctx):
    c = ac.case("room_color")
    create(ctx, c)
    d0, d1 = c["frames"]
    i0, i1 = c["intensities"]
    p0 = c["ops"][1][2]
    run(ctx, c, [(+1, 0, p0), (+1, 1, p0)])
    before = ctx.tsdf_get(intensity=True)
    kw = dict(fx=c["fx"], cx=c["cx"])
    bad_pose = p0.copy()
    bad_pose[1, 3] = np.inf
    bad_inten = i0.copy()
    bad_inten[3, 4] = 1.25
    refused = [
        lambda: binding.tsdf_apply(ctx, [d0], [], [i0], **kw),                                  # n_ops < 1
        lambda: binding.tsdf_apply(ctx, [d0], [(+1, 0, p0)] * 17, [i0], **kw),                  # n_ops > 16
        lambda: binding.tsdf_apply(ctx, [d0, d1], [(+1, 0, p0)], [i0, i1], **kw),               # n_frames > n_ops
        lambda: binding.tsdf_apply(ctx, [d0], [(+1, 0, p0), (0, 0, p0)], [i0], **kw),           # a sign that is neither
        lambda: binding.tsdf_apply(ctx, [d0], [(+1, 0, p0), (-2, 0, p0)], [i0], **kw),
        lambda: binding.tsdf_apply(ctx, [d0], [(+1, 0, p0), (-1, 1, p0)], [i0], **kw),          # a frame out of range
        lambda: binding.tsdf_apply(ctx, [d0], [(+1, -1, p0)], [i0], **kw),
        lambda: binding.tsdf_apply(ctx, [d0], [(-1, 0, bad_pose)], [i0], **kw),                 # a pose that is not finite
        lambda: binding.tsdf_apply(ctx, [d0], [(-1, 0, p0)], None, **kw),                       # colour without intensities
        lambda: binding.tsdf_apply(ctx, [d0], [(-1, 0, p0)], [bad_inten], **kw),                # an intensity out of range
        lambda: binding.tsdf_apply(ctx, [d0], [(-1, 0, p0)], [i0], fx=0.0, cx=c["cx"]),         # what integrate refuses
        lambda: binding.tsdf_apply(ctx, [d0], [(-1, 0, p0)], [i0], fx=c["fx"], cx=np.nan),
        lambda: binding.tsdf_deintegrate(ctx, d0, bad_pose, i0, **kw),
        lambda: binding.tsdf_deintegrate(ctx, d0, p0, None, **kw),
    ]
    for k, call in enumerate(refused):
        with pytest.raises(binding.IcpkError) as e:
            call()
        assert e.value.code == binding.E_ARG, k
    # n_frames < 1, a NULL frame, a NULL op list: below the binding
    import ctypes as C
    u16, fp = C.POINTER(C.c_uint16), C.POINTER(C.c_float)
    ops = binding.tsdf_ops([(-1, 0, p0), (+1, 1, p0)])
    dt = (u16 * 2)(d0.ctypes.data_as(u16), None)
    it = (fp * 2)(i0.ctypes.data_as(fp), i1.ctypes.data_as(fp))
    rows, cols = d0.shape
    lib, h = ctx._lib, ctx._h
    assert lib.icpk_tsdf_apply(h, 0, dt, it, rows, cols, c["fx"], c["cx"], 2, ops, None) == binding.E_ARG
    assert lib.icpk_tsdf_apply(h, 2, dt, it, rows, cols, c["fx"], c["cx"], 2, ops, None) == binding.E_ARG
    assert lib.icpk_tsdf_apply(h, 1, None, it, rows, cols, c["fx"], c["cx"], 2, ops, None) == binding.E_ARG
    assert lib.icpk_tsdf_apply(h, 1, dt, it, rows, cols, c["fx"], c["cx"], 2, None, None) == binding.E_ARG
    assert lib.icpk_tsdf_apply(h, 1, dt, it, 0, cols, c["fx"], c["cx"], 2, ops, None) == binding.E_ARG
    assert same_planes(ctx.tsdf_get(intensity=True), before)
    # intensities on a volume without colour; and no volume at all
    create(ctx, ac.case("room"))
    with pytest.raises(binding.IcpkError) as e:
        binding.tsdf_apply(ctx, [d0], [(+1, 0, p0)], [i0], **kw)
    assert e.value.code == binding.E_ARG and not ctx.tsdf_get()[1].any()
    ctx.tsdf_release()
    for call in (lambda: binding.tsdf_apply(ctx, [d0], [(+1, 0, p0)], None, **kw), lambda: binding.tsdf_deintegrate(ctx, d0, p0, **kw)):
        with pytest.raises(binding.IcpkError) as e:
            call()
        assert e.value.code == binding.E_NOT_SET


def test_apply_leaves_the_surface_the_raycast_and_the_frame_view_alone(ctx):
    c = ac.case("room_color")
    create(ctx, c)
    d0, d1 = c["frames"]
    p0, p1 = c["ops"][1][2], c["ops"][2][2]
    run(ctx, c, [(+1, 0, p0), (+1, 1, p1)])
    n_surf = ctx.tsdf_extract_surface(1)
    ctx.tsdf_raycast(p0, shape=d0.shape, fx=c["fx"], cx=c["cx"], z_near=0.25, z_far=6.0, min_weight=1)
    n_mesh = ctx.tsdf_extract_mesh(1)
    depth_front.build_pyramid(ctx, d1)
    binding.frame_view_build(ctx, p1, fx=c["fx"], cx=c["cx"])

    def snapshot():
        s, r, m = ctx.tsdf_get_surface(), ctx.tsdf_get_raycast(), ctx.tsdf_get_mesh()
        out = [s[k] for k in sorted(s)] + [r[k] for k in sorted(r)] + [m[k] for k in sorted(m) if isinstance(m[k], np.ndarray)]
        out += [binding.frame_view(ctx, l) for l in range(binding.frame_view_levels(ctx))]
        return out + [depth_front.pyramid_level(ctx, 0)]

    before = snapshot()
    assert n_surf[0] > 1000 and n_mesh[0] > 1000 and (before[-1] == d1).all()
    n = run(ctx, c, [(-1, 1, p1), (+1, 1, ac.drift(p1, (0.0, 3.0, 0.0), (0.05, 0.0, 0.0))), (-1, 0, p0)])
    assert n.min() > 1000
    after = snapshot()
    assert len(before) == len(after) and all(same_bits(np.asarray(x), np.asarray(y)) for x, y in zip(before, after))


def test_a_reused_context_gives_a_fresh_contexts_bytes(ctx):
    """after calls of other shapes and other n_frames the frame stack and the counts carry nothing over"""
    want = {}
    for name in ("tiny", "room_color", "tail"):
        with binding.Context(0) as fresh:
            c = ac.case(name)
            create(fresh, c)
            want[name] = (run(fresh, c).tolist(), planes(fresh, c))
    big = tc.room_frame(*tc.ROOM_MOTIONS[0], shape=(240, 320), fx=2 * tc.ROOM_FX, cx=2 * tc.ROOM_CX + 0.5)
    for name in ("room_color", "tiny", "tail", "room_color"):
        c = ac.case(name)
        create(ctx, c)
        got = run(ctx, c).tolist()
        assert got == want[name][0] and same_planes(planes(ctx, c), want[name][1]), name
        # a larger frame, alone, on a volume without colour in between: the stack grows and is reused
        create(ctx, ac.case("room"))
        binding.tsdf_apply(ctx, [big[0]], [(+1, 0, big[1])], None, fx=2 * tc.ROOM_FX, cx=2 * tc.ROOM_CX + 0.5)


def test_refuse_moves_frames_in_batches_of_eight(ctx):
    """eleven frames (two batches: 8 and 3) fused at drifted poses and moved to the true ones: the weight plane is that
    of the frames fused at the true poses, and the per-frame counts are the model's"""
    c = tc.case("room")
    frames = [tc.room_frame((0.0, 2.0 * k - 10.0, 0.0), (0.02 * k, 0.0, 0.0)) for k in range(11)]
    depths, true = [f[0] for f in frames], [f[1] for f in frames]
    old = [ac.drift(P, (0.3 * k, -0.2 * k, 0.0), (0.004 * k, 0.0, -0.003 * k)) for k, P in enumerate(true)]
    kw = {k: c["volume"][k] for k in ("dims", "voxel", "origin", "trunc")}
    vol = TsdfVolume(ctx, fx=c["fx"], cx=c["cx"], **kw)
    added_old = vol.integrate_all(depths, old)
    moved = vol.refuse(depths, old, true)
    assert vol.frames == 11 and moved.shape == (11, 2)
    f, w, _ = vol.planes()
    ref = TsdfVolume(ctx, fx=c["fx"], cx=c["cx"], **kw)
    added_true = ref.integrate_all(depths, true)
    g, v, _ = ref.planes()
    assert same_bits(w, v) and w.max() == 11
    assert moved[:, 0].tolist() == added_old and moved[:, 1].tolist() == added_true
    # 11 frames in, then 8 out and in, then 3 out and in: the worst a voxel can carry whichever of those ops hit it,
    # against the worst of 11 frames in
    bound = (am.any_subsequence_error_bound([+1] * 11 + [-1] * 8 + [+1] * 8 + [-1] * 3 + [+1] * 3) +
             am.any_subsequence_error_bound([+1] * 11)) * am.EPS
    diff = np.abs(f.astype(np.float64) - g.astype(np.float64)).max()
    print(f"refuse: max |diff| {diff:.3g}, bound {bound:.3g}")
    assert diff <= bound
