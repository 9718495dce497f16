"""The cases of K26 shared by tests/test_projective_color_host.py, tests/test_gpu_projective_color.py and the thread test:
colour volumes, views of them with their gradients, frames with an intensity image, and the wall the feature is for.
Every model run is computed once per process and handed out read-only."""
import functools
import zlib

import numpy as np

import color_model as cm
import projective_cases as pc
import projective_color_model as km
import projective_model as jm
import pyramid_model as pm
import tsdf_cases as tc
import tsdf_model
import tsdf_raycast_cases as rc
import tsdf_raycast_model as rm
from icp_slam_prototype_amd import synth

F = np.float32


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def texture(x, y):
    """K17's wall texture of a point"""
    return 0.5 + 0.25 * np.sin(2 * np.pi * x / 0.2) + 0.2 * np.cos(2 * np.pi * y / 0.15)


# ---- the intensity pyramid --------------------------------------------------------------------------------------------
# name -> (case of pyramid_model or "room_color" / "room_color_masked", levels)
PYRAMID_CASES = {"1x1": 3, "1x40": 3, "40x1": 3, "3x3": 3, "17x65": 4, "68x260": 8, "room_color": 3, "room_color_masked": 4,
                 "cutoff_1": 3, "half_planes_odd": 3, "half_planes_even": 3}


@functools.lru_cache(maxsize=None)
def pyramid_case(name):
    """(depth uint16, intensity float32 in [0, 1], K, levels); read-only"""
    rng = _rng("pyr" + name)
    if name.startswith("room_color"):
        d, _, inten = tc.case("room_color")["frames"][1]
        d, K = np.array(d), pm.DEFAULT_K
        if name.endswith("masked"):
            d[rng.random(d.shape) < 0.3] = 0
        inten = np.array(inten, F)
    else:
        d, K = pm.case(name)
        inten = rng.random(d.shape).astype(F)
        if name.startswith("half_planes"):  # 0.25 on the near side, 0.75 on the far side: nothing may cross the step
            inten = np.where(d == d.min(), F(0.25), F(0.75)).astype(F)
    inten[0, 0] = 1.0  # (both ends of the range occur)
    inten[-1, -1] = 0.0
    for a in (d, inten):
        a.setflags(write=False)
    return d, inten, K, PYRAMID_CASES[name]


@functools.lru_cache(maxsize=None)
def pyramid_expected(name):
    d, inten, K, levels = pyramid_case(name)
    out = km.intensity_pyramid(d, inten, levels, K)
    for a in out:
        a.setflags(write=False)
    return out


# ---- colour volumes ---------------------------------------------------------------------------------------------------
def _plane_intensity():
    """the wall texture over the `plane` case's frame (fx 64, cx 31.5, z 1.5)"""
    v, u = np.mgrid[0:48, 0:64].astype(np.float64)
    return texture((u - 31.5) * 1.5 / 64.0, (v - 31.5) * 1.5 / 64.0).astype(F)


@functools.lru_cache(maxsize=None)
def volume_case(name):
    """dict(volume keywords, fx, cx, frames [(depth, pose, intensity)]) of a COLOUR volume"""
    if name == "room_color":
        return tc.case("room_color")
    if name == "plane_wall":
        c = tc.case("plane")
        d, P, _ = c["frames"][0]
        return dict(c, volume=dict(c["volume"], color=True), frames=[(d, P, _plane_intensity())])
    if name == "holes_color":
        c = tc.case("holes")
        d, P, _ = c["frames"][0]
        return dict(c, volume=dict(c["volume"], color=True), frames=[(d, P, tc.room_intensity(*tc.ROOM_MOTIONS[1]))])
    if name == "wall":
        w = wall()
        return dict(volume=dict(WALL_VOLUME, color=True), fx=WALL_FX, cx=WALL_CX, frames=[(w["frames"][0][0], w["poses"][0], w["frames"][0][1])])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def volume_model(name):
    c = volume_case(name)
    if name == "room_color":
        return tc.model("room_color")["volume"]
    vol = tsdf_model.Volume(**c["volume"])
    for d, P, inten in c["frames"]:
        vol.integrate(d, P, c["fx"], c["cx"], inten)
    return vol


def create_volume(ctx, binding, name):
    """the colour volume of a case fused on the context"""
    c = volume_case(name)
    v = c["volume"]
    ctx.tsdf_create(dims=v["dims"], voxel=v["voxel"], origin=v["origin"], trunc=v["trunc"], max_weight=v.get("max_weight"),
                    flags=binding.TSDF_COLOR)
    for d, P, inten in c["frames"]:
        ctx.tsdf_integrate(d, P, inten, fx=c["fx"], cx=c["cx"])


@functools.lru_cache(maxsize=None)
def view_maps(volume, pose_key, view_key):
    pose = np.frombuffer(pose_key, np.float64).reshape(4, 4)
    maps = rm.raycast(volume_model(volume), pose, **dict(view_key))["maps"]
    maps.setflags(write=False)
    return maps


def _maps(volume, pose, view):
    return view_maps(volume, np.asarray(pose, np.float64).tobytes(), tuple(sorted(view.items())))


# ---- the view gradients -----------------------------------------------------------------------------------------------
def _room_view(shape):
    return dict(rc.ROOM_VIEW, shape=shape, fx=tc.ROOM_FX * shape[1] / tc.ROOM_SHAPE[1], cx=(shape[1] - 1) / 2.0)


P4 = lambda: tc.pose(*tc.ROOM_FOURTH)
# name -> (colour volume, view pose, view keywords, radius, min_neighbors)
GRADIENT_CASES = {
    "1x1": ("room_color", P4, _room_view((1, 1)), 0.125, 1),
    "1x5": ("room_color", P4, _room_view((1, 5)), 2.0, 2),
    "7x9": ("room_color", P4, _room_view((7, 9)), 1.0, 4),
    "17x65": ("room_color", P4, _room_view((17, 65)), 0.25, 4),
    "plane_wall": ("plane_wall", lambda: np.eye(4), rc.PLANE_VIEW, 0.125, 4),
    "room_color": ("room_color", P4, rc.ROOM_VIEW, 0.125, 4),
    # a radius below the pixel spacing: only the centre counts, m = 1 and no gradient anywhere
    "room_tiny_radius": ("room_color", P4, rc.ROOM_VIEW, 1e-4, 1),
    # all nine neighbours asked for: pixels beside a hole or a depth step get none
    "room_min_nb_9": ("room_color", P4, rc.ROOM_VIEW, 0.125, 9),
    # the one-frame volume with holes: few hits, most of them with holes around them
    "holes_color": ("holes_color", lambda: tc.case("holes")["frames"][0][1], dict(rc.ROOM_VIEW, step=0.15), 0.3, 2),
}


@functools.lru_cache(maxsize=None)
def gradient_case(name):
    """dict(volume, pose, view, radius, min_neighbors, maps (8, rows, cols), gradients (3, rows, cols), sums (n, 10))"""
    volume, pose, view, radius, min_nb = GRADIENT_CASES[name]
    P = np.asarray(pose(), np.float64)
    maps = _maps(volume, P, view)
    g, S = km.view_gradients(maps, radius, min_nb)
    for a in (g, S):
        a.setflags(write=False)
    return dict(volume=volume, pose=P, view=view, radius=radius, min_neighbors=min_nb, maps=maps, gradients=g, sums=S)


def check_gradient_conditions():
    """what the gradient cases are for, asserted on the model's output"""
    room = gradient_case("room_color")
    hit = room["maps"][6].reshape(-1) > 0
    m = room["sums"][:, 0]
    assert hit.any() and not hit.all() and (m[~hit] == 0).all() and not room["gradients"].reshape(3, -1)[:, ~hit].any()
    assert ((m[hit] < 9) & (m[hit] > 1)).any()  # hit pixels with holes (or depth steps) among their neighbours
    assert (room["gradients"] != 0).any()
    tiny = gradient_case("room_tiny_radius")
    assert (tiny["sums"][hit, 0] == 1).all() and not tiny["sums"][:, 1:].any() and not tiny["gradients"].any()
    nine = gradient_case("room_min_nb_9")
    gn = (nine["gradients"] != 0).any(0).reshape(-1)
    assert gn.any() and (nine["sums"][gn, 0] == 9).all() and ((m == 9) | ~gn).all()
    assert (gradient_case("plane_wall")["gradients"] != 0).any()


def synthetic_view(rows=9, cols=11, seed=3):
    """A view no ray cast gives (K20 lists only crossings that have a normal), for the host function alone: a slanted
    plane with holes, hit pixels whose normal is zero, one whose normal is grossly non-unit and one NaN point."""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:rows, 0:cols].astype(np.float64)
    z = 1.0 + 0.02 * u + 0.01 * v
    n = np.array([-0.02, -0.01, 1.0])
    n /= np.linalg.norm(n)
    maps = np.zeros((8, rows, cols), F)
    maps[0], maps[1], maps[2] = 0.03 * u, 0.03 * v, z
    maps[3], maps[4], maps[5] = n[0], n[1], n[2]
    maps[6] = z
    maps[7] = rng.random((rows, cols))
    hole = rng.random((rows, cols)) < 0.2
    hole[4, 5] = hole[2, 2] = hole[6, 7] = hole[3, 8] = False
    maps[:, hole] = 0
    maps[3:6, 4, 5] = 0            # a hit with the zero normal: m kept, nine zero sums, no gradient
    maps[3:6, 2, 2] *= 1.5         # not usable either
    maps[0, 6, 7] = np.nan         # a point nobody is a neighbour of, itself included
    maps.setflags(write=False)
    return maps


# ---- the joint reduction: K25's cases over colour volumes -------------------------------------------------------------
COLOR_VOLUME = {"room": "room_color", "plane": "plane_wall", "holes": "holes_color"}
NAMES = pc.NAMES
LOOP_CASES = pc.LOOP_CASES
LAMBDAS = (0.0, 0.5, 0.968, 1.0)


@functools.lru_cache(maxsize=None)
def case(name):
    """projective_cases.case(name) over the colour volume of the same geometry, with an intensity image of the frame
    (the room's own for the room frames, uniform noise otherwise), the level's intensities, and the gradient settings"""
    c = dict(pc.case(name))
    c["volume"] = COLOR_VOLUME[c["volume"]]
    d = c["depth"]
    if name in ("room_l0", "room_l1", "room_yaw30", "too_far", "normal_gate"):
        inten = tc.room_intensity(*tc.ROOM_FOURTH)
    else:
        inten = _rng("frame" + name).random(d.shape).astype(F)
    inten = np.ascontiguousarray(inten, F)
    c["intensity"] = inten
    c["level_intensity"] = km.intensity_pyramid(d, inten, c["level"] + 1)[c["level"]]
    voxel = volume_case(c["volume"])["volume"]["voxel"]
    c["radius"], c["min_neighbors"] = 2.0 * voxel, 4
    for a in (c["intensity"], c["level_intensity"]):
        a.setflags(write=False)
    return c


def maps_of(name):
    c = case(name)
    return _maps(c["volume"], c["view_pose"], c["view"])


@functools.lru_cache(maxsize=None)
def gradients_of(name):
    c = case(name)
    g, _ = km.view_gradients(maps_of(name), c["radius"], c["min_neighbors"])
    g.setflags(write=False)
    return g


def model_args(name, pose=None, lambda_geometric=cm.LAMBDA):
    c = case(name)
    v = c["view"]
    return dict(level=c["level_image"], level_intensity=c["level_intensity"], fx_s=c["fx_s"], cx_s=c["cx_s"], view=maps_of(name),
                gradient=gradients_of(name), view_shape=v["shape"], fx_v=v["fx"], cx_v=v["cx"], view_pose=c["view_pose"],
                pose=c["estimate"] if pose is None else pose, max_dist=c["max_dist"], min_normal_cos=c["min_normal_cos"],
                lambda_geometric=lambda_geometric)


@functools.lru_cache(maxsize=None)
def expected(name, lambda_geometric=cm.LAMBDA):
    out = km.pixels(**model_args(name, lambda_geometric=lambda_geometric))
    out["sums"], out["count"] = km.reduce(out["terms"], out["pixel"])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_geometric(name):
    """K25's model on the colour volume's maps (the same geometry as K25's own cases)"""
    a = model_args(name)
    out = jm.pixels(a["level"], a["fx_s"], a["cx_s"], a["view"], a["view_shape"], a["fx_v"], a["cx_v"], a["view_pose"], a["pose"],
                    a["max_dist"], a["min_normal_cos"])
    out["sums"], out["count"] = jm.reduce(out["terms"], out["pixel"])
    return out


def check_conditions():
    """counts and codes are K25's; zero gradients are mixed in among the pairs of the room"""
    for name in NAMES:
        e, k25 = expected(name), pc.expected(name)
        assert e["pixel"].tobytes() == k25["pixel"].tobytes() and e["count"] == k25["count"], name
    e = expected("room_l0")
    pair = e["pixel"] >= 0
    g = gradients_of("room_l0").reshape(3, -1)[:, e["pixel"][pair]]
    zero = ~(g != 0).any(0)
    assert zero.any() and not zero.all(), (int(zero.sum()), int(pair.sum()))


def device_setup(ctx, name, depth_front, binding, gradients=True, intensity=True):
    """The case on a context: the colour volume fused, the view ray-cast, its gradients made, the frame's pyramid built and
    its intensity set.  Returns the ProjectiveParams of the case."""
    c = case(name)
    create_volume(ctx, binding, c["volume"])
    ctx.tsdf_raycast(c["view_pose"], **c["view"])
    if gradients:
        binding.raycast_color_gradients(ctx, c["radius"], c["min_neighbors"])
    depth_front.build_pyramid(ctx, c["depth"], depth_front.pyramid_params(levels=c["level"] + 1))
    if intensity:
        binding.set_pyramid_intensity(ctx, c["intensity"])
    return binding.default_projective_params(level=c["level"], fx=c["fx"], cx=c["cx"], max_dist=c["max_dist"],
                                             min_normal_cos=c["min_normal_cos"])


# ---- the wall: the claim the feature makes ----------------------------------------------------------------------------
# An exact plane at z = 1 m, fronto-parallel, seen by a 60 x 80 camera of fx = 60: a pixel covers 16.7 mm of the wall
# and a voxel 25 mm, so the texture's wavelengths (200 and 150 mm) are 12 and 9 pixels, 8 and 6 voxels.
WALL_SHAPE, WALL_FX, WALL_CX, WALL_Z = (60, 80), 60.0, 39.5, 1.0
WALL_VOLUME = dict(dims=(64, 48, 16), voxel=0.025, origin=(-0.7875, -0.5875, 0.8125), trunc=0.1)
WALL_VIEW = dict(shape=WALL_SHAPE, fx=WALL_FX, cx=WALL_CX, z_near=0.25, z_far=3.0, step=0.05, min_weight=1)
WALL_MOTION = ((0.030, -0.020, 0.004), 1.0)  # in the plane by (30, -20) mm, 4 mm along the normal, 1 degree about it
WALL_ITER, WALL_MAX_DIST, WALL_RADIUS, WALL_MIN_NB = 20, 0.5, 0.05, 4
# measured with the numpy models (tests/test_projective_color_host.py prints them): rotation (Frobenius),
# translation (m) of the coloured loop after 20 iterations at level 0.  The condition the claim stands on: the
# translation error is below a quarter of the in-plane motion (36.06 mm / 4 = 9 mm).
WALL_MEASURED = (0.0005537285607238006, 0.0049782010656580465)
WALL_CONDITION = 0.25 * float(np.hypot(0.030, 0.020))


@functools.lru_cache(maxsize=None)
def wall():
    """dict(poses [P0, P1], frames [(depth, intensity)] x 2)"""
    a = np.deg2rad(WALL_MOTION[1])
    P1 = np.eye(4)
    P1[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    P1[:3, 3] = WALL_MOTION[0]
    poses = [np.eye(4), P1]
    frames = synth.textured_wall_frames(poses, *WALL_SHAPE, fx=WALL_FX, cx=WALL_CX, z=WALL_Z, relief=0.0)
    for d, i in frames:
        d.setflags(write=False)
        i.setflags(write=False)
    return dict(poses=poses, frames=frames)


@functools.lru_cache(maxsize=None)
def wall_model():
    """The wall on the models: dict(maps, gradients, colored: the coloured loop's result, geometric: K25's)"""
    w = wall()
    P0 = w["poses"][0]
    maps = _maps("wall", P0, WALL_VIEW)
    g, _ = km.view_gradients(maps, WALL_RADIUS, WALL_MIN_NB)
    d1, i1 = w["frames"][1]
    geo = dict(fx_s=F(WALL_FX), cx_s=F(WALL_CX), view=maps, view_shape=WALL_SHAPE, fx_v=WALL_FX, cx_v=WALL_CX, view_pose=P0, pose=P0,
               max_dist=WALL_MAX_DIST)
    colored = km.align(max_iterations=WALL_ITER, level=d1, level_intensity=i1, gradient=g, **geo)
    geometric = jm.align(level=d1, max_iterations=WALL_ITER, **geo)
    return dict(maps=maps, gradients=g, colored=colored, geometric=geometric)


def wall_errors(pose):
    return cm.pose_errors(pose, wall()["poses"][1])
