"""The small cases of the SDF tracking rule (K29) shared by tests/test_sdf_track_host.py and tests/test_gpu_sdf_track.py:
a volume of tsdf_cases (or one set by hand), a frame of projective_cases, a level of the frame's pyramid and an estimate.
Every model run is computed once per process and handed out read-only."""
import functools

import numpy as np

import projective_cases as pc
import pyramid_model as pm
import sdf_track_model as sm
import tsdf_cases as tc
import tsdf_model
import tsdf_shift_model as shm

P3 = pc.P3
SHIFT = (3, -2, 1)  # the `shifted` case: icpk_tsdf_shift by these voxels


def _constant_volume():
    """the plane case's geometry with every voxel at 0.5, weight 1: the interpolant has no gradient anywhere"""
    v = tsdf_model.Volume(**tc.case("plane")["volume"])
    v.tsdf[:] = 0.5
    v.weight[:] = 1
    return v


ROOM = dict(volume="room", fx=tc.ROOM_FX, cx=tc.ROOM_CX, level=0, estimate=P3, frame=pc.CASES["room_l0"]["frame"])
PLANE = dict(volume="plane", fx=64.0, cx=31.5, level=0, estimate=pc.PLANE_SHIFT, frame=pc.PLANE["frame"])

# name -> dict(volume: case of tsdf_cases or "constant", frame: the level-0 depth image, fx, cx: its LEVEL-0 intrinsics,
# level, estimate, shift (voxels, or absent), the gates where they are not the defaults; min_pairs: what the case is known
# to have at least -- 6 unless the case cannot have them)
CASES = {
    # 120 x 160, 19 200 pixels, 75 workgroups
    "room_l0": ROOM,
    # level 1 (60 x 80)
    "room_l1": dict(ROOM, level=1),
    # tiny sources: one pixel (at most one accepted), and two that fill no wave
    "1x1": dict(ROOM, **{k: pc.CASES["1x1"][k] for k in ("frame", "fx", "cx")}, min_pairs=1),
    "7x9": dict(ROOM, **{k: pc.CASES["7x9"][k] for k in ("frame", "fx", "cx")}),
    "17x19": dict(ROOM, **{k: pc.CASES["17x19"][k] for k in ("frame", "fx", "cx")}),
    # 260 x 260 of constant depth on the plane volume: 67 600 pixels, more than 256 x 256, so the first lanes take two
    "260x260": dict(PLANE, frame=pc.CASES["260x260"]["frame"], fx=260.0, cx=129.5),
    # an estimate 50 m away: every point is OUTSIDE
    "outside": dict(ROOM, estimate=lambda: tc.pose(tc.ROOM_MOTIONS[2][0], (50.0, 0.0, 0.0)), min_pairs=0),
    # the one-frame volume with holes, and its frame with holes: UNKNOWN (and NO_DEPTH)
    "holes": dict(volume="holes", fx=tc.ROOM_FX, cx=tc.ROOM_CX, level=0, frame=lambda: tc.case("holes")["frames"][0][0],
                  estimate=lambda: tc.case("holes")["frames"][0][1]),
    # a tighter max_abs_tsdf: TOO_FAR
    "too_far": dict(ROOM, max_abs_tsdf=0.0625),
    # a constant 0.5 at weight 1, set by icpk_tsdf_set: NO_GRADIENT wherever the point is in range
    "constant": dict(PLANE, volume="constant", estimate=lambda: np.eye(4), min_pairs=0),
    # the normal gate on the noisy room: NO_NORMAL (the border, a hole beside the pixel) and NORMAL
    "normal_gate": dict(ROOM, frame=pc.CASES["normal_gate"]["frame"], min_normal_cos=0.9),
    # the fronto-parallel plane at its true pose: its normal equations are degenerate
    "plane": dict(PLANE, estimate=lambda: np.eye(4)),
    # the room volume after icpk_tsdf_shift: the shifted origin is the one read
    "shifted": dict(ROOM, shift=SHIFT),
}
NAMES = tuple(CASES)
LOOP_CASES = ("room_l0", "room_l1")  # the 10-iteration runs checked by their traces


@functools.lru_cache(maxsize=None)
def base_volume(name):
    """the tsdf_model.Volume a case starts from, before any shift (read-only planes)"""
    if name == "constant":
        v = _constant_volume()
        v.tsdf.setflags(write=False)
        v.weight.setflags(write=False)
        return v
    return tc.model(name)["volume"]


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(volume: its name, base: the Volume before the shift, vol: the Volume the rule reads (shifted where the case
    says so: moved planes and the origin by K23's rule), shift, depth: the level-0 frame, level_image, level, fx, cx
    (level 0), fx_s, cx_s (the level's), estimate (4, 4), max_abs_tsdf, min_weight, min_normal_cos, min_pairs)"""
    c = CASES[name]
    depth = np.ascontiguousarray(c["frame"](), np.uint16)
    level = c["level"]
    img = pm.pyramid(depth, level + 1)[level]
    for a in (depth, img):
        a.setflags(write=False)
    base = base_volume(c["volume"])
    shift = c.get("shift")
    vol = base if shift is None else shm.shifted(base, shift)
    if shift is not None:
        vol.tsdf.setflags(write=False)
        vol.weight.setflags(write=False)
    scale = np.float32(2 ** level)
    return dict(volume=c["volume"], base=base, vol=vol, shift=shift, depth=depth, level_image=img, level=level, fx=c["fx"],
                cx=c["cx"], fx_s=np.float32(c["fx"]) / scale, cx_s=np.float32(c["cx"]) / scale,
                estimate=np.asarray(c["estimate"](), np.float64), max_abs_tsdf=c.get("max_abs_tsdf", 1.0),
                min_weight=c.get("min_weight", 1), min_normal_cos=c.get("min_normal_cos", -2.0), min_pairs=c.get("min_pairs", 6))


def model_args(name, pose=None):
    """the arguments of sdf_track_model.pixels / align for a case (pose: default the case's estimate)"""
    c = case(name)
    return dict(level=c["level_image"], fx_s=c["fx_s"], cx_s=c["cx_s"], vol=c["vol"], pose=c["estimate"] if pose is None else pose,
                max_abs_tsdf=c["max_abs_tsdf"], min_weight=c["min_weight"], min_normal_cos=c["min_normal_cos"])


@functools.lru_cache(maxsize=None)
def expected(name):
    """The model at the case's estimate: dict(cell, value, terms, sums, count); arrays are read-only."""
    out = sm.pixels(**model_args(name))
    out["sums"], out["count"] = sm.reduce(out["terms"], out["cell"])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_loop(name, max_iterations=10):
    return sm.align(max_iterations=max_iterations, **model_args(name))


def check_conditions():
    """What the cases are for, asserted on the model's output alone: every code occurs somewhere, and every case has the
    accepted pixels (or the rejections) it claims."""
    seen = {}
    for name in NAMES:
        e = expected(name)
        seen[name] = set(int(v) for v in np.unique(e["cell"]) if v < 0)
        assert e["count"] >= case(name)["min_pairs"], (name, e["count"])
        ok = e["cell"] >= 0
        assert (e["cell"][ok] < 2 ** 30).all() and (e["value"][~ok] == 0).all(), name
    assert set().union(*seen.values()) == set(sm.CODES), sorted(set().union(*seen.values()))
    assert expected("1x1")["count"] == 1
    assert (expected("outside")["cell"] == sm.OUTSIDE).all()
    assert sm.UNKNOWN in seen["holes"] and sm.NO_DEPTH in seen["holes"]
    # the tighter gate rejects pixels the default accepts, and nothing else changes
    a, b = expected("room_l0")["cell"], expected("too_far")["cell"]
    assert (b == sm.TOO_FAR).sum() > (a == sm.TOO_FAR).sum() and ((b == a) | (b == sm.TOO_FAR)).all()
    c = expected("constant")["cell"]
    assert set(np.unique(c)) == {sm.OUTSIDE, sm.NO_GRADIENT} and expected("constant")["count"] == 0
    assert {sm.NO_NORMAL, sm.NORMAL} <= seen["normal_gate"]
    assert expected("260x260")["cell"].size == 67600 > 256 * 256
    assert expected_loop("constant", 4)["status"] == sm.W_TOO_FEW_PAIRS
    assert expected_loop("plane", 4)["status"] == sm.W_DEGENERATE and expected("plane")["count"] >= 6
    # the shifted volume is read at the shifted origin: the same world points, cells SHIFT away, the values of room_l0
    # wherever both are accepted (the origin moves by a rounded sum, so a fraction may differ in its last bits)
    s, r = expected("shifted"), expected("room_l0")
    both = (s["cell"] >= 0) & (r["cell"] >= 0)
    dims = case("room_l0")["vol"].dims
    step = SHIFT[0] + dims[0] * (SHIFT[1] + dims[1] * SHIFT[2])
    assert both.sum() > 1000 and (np.abs(s["value"][both] - r["value"][both]) < 1e-4).all()
    assert np.mean(r["cell"][both] - s["cell"][both] == step) > 0.99
    assert not np.array_equal(case("shifted")["vol"].origin, case("room_l0")["vol"].origin)


def volume_params(name, binding):
    """the TsdfParams of the volume the rule reads, with the origin to use"""
    v = case(name)["vol"]
    return binding.tsdf_params(dims=v.dims, voxel=float(v.voxel), origin=[float(x) for x in v.origin], trunc=float(v.trunc))


def sdf_params(name, binding, **kw):
    c = case(name)
    return binding.default_sdf_params(**dict(dict(level=c["level"], fx=c["fx"], cx=c["cx"], max_abs_tsdf=c["max_abs_tsdf"],
                                                  min_weight=c["min_weight"], min_normal_cos=c["min_normal_cos"]), **kw))


def device_setup(ctx, name, depth_front, binding):
    """The case on a context: the volume created and set to the base planes, shifted on the device where the case says
    so, the frame's pyramid built.  Returns the SdfParams of the case."""
    c = case(name)
    b = c["base"]
    ctx.tsdf_create(dims=b.dims, voxel=float(b.voxel), origin=[float(x) for x in b.origin], trunc=float(b.trunc))
    ctx.tsdf_set(b.tsdf, b.weight)
    if c["shift"] is not None:
        binding.tsdf_shift(ctx, c["shift"])
    depth_front.build_pyramid(ctx, c["depth"], depth_front.pyramid_params(levels=c["level"] + 1))
    return sdf_params(name, binding)
