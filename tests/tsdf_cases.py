"""The small TSDF cases (K19) shared by tests/test_tsdf_host.py and tests/test_gpu_tsdf.py: volume parameters, frames,
poses.  Every model volume is computed once per process and handed out read-only."""
import functools

import numpy as np

import tsdf_model
from icp_slam_prototype_amd import synth

ROOM_FX, ROOM_CX = 117.15, 79.5
ROOM_SHAPE = (120, 160)
ROOM_MOTIONS = [((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), ((0.0, 4.0, 0.0), (0.06, 0.0, 0.0)),
                ((2.0, -4.0, 0.0), (-0.05, 0.03, 0.02))]
ROOM_FOURTH = ((1.0, 2.0, 0.0), (0.03, 0.01, 0.01))  # a further frame, aligned against the model
ROOM_VOLUME = dict(dims=(64, 64, 64), voxel=0.0625, origin=(-2.3, -1.9, 0.4), trunc=0.25)


def pose(rot_deg, shift):
    """camera-to-world: the rotation and centre synth.render_room_depth takes"""
    P = np.eye(4)
    P[:3, :3] = synth.rot_xyz_deg(*rot_deg)
    P[:3, 3] = shift
    return P


def room_frame(rot_deg, shift, shape=ROOM_SHAPE, fx=ROOM_FX, cx=ROOM_CX):
    P = pose(rot_deg, shift)
    return synth.render_room_depth(shape[0], shape[1], P[:3, :3], P[:3, 3], fx, cx), P


def room_intensity(rot_deg, shift, shape=ROOM_SHAPE, fx=ROOM_FX, cx=ROOM_CX):
    P = pose(rot_deg, shift)
    bgr = synth.render_room_color(shape[0], shape[1], P[:3, :3], P[:3, 3], fx, cx)
    return (bgr.astype(np.float64).sum(-1) / 765.0).astype(np.float32)  # (icpk_intensity_from_bgr's formula)


def room_distance(p):
    """distance of the points (3, n) to the analytic room of synth.py: floor, back wall, left wall, sphere"""
    p = np.asarray(p, np.float64)
    sphere = np.abs(np.linalg.norm(p - np.array([[0.35], [0.45], [2.3]]), axis=0) - 0.55)
    return np.minimum.reduce([np.abs(p[1] - 1.3), np.abs(p[2] - 3.6), np.abs(p[0] + 2.1), sphere])


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(volume (keywords of tsdf_model.Volume / TsdfParams fields), fx, cx, frames: list of (depth, pose,
    intensity or None))"""
    if name in ("room", "room_color"):
        color = name == "room_color"
        frames = []
        for rot, shift in ROOM_MOTIONS:
            d, P = room_frame(rot, shift)
            frames.append((d, P, room_intensity(rot, shift) if color else None))
        return dict(volume=dict(ROOM_VOLUME, color=color), fx=ROOM_FX, cx=ROOM_CX, frames=frames)
    if name == "odd":
        # 33 x 17 x 9 over the left wall and the floor; the camera stands inside the volume and is turned towards the
        # wall, so that a third of the voxels lie behind it and another third project outside the image
        d, P = room_frame((20.0, 50.0, 0.0), (-0.3, 0.5, 1.1))
        return dict(volume=dict(dims=(33, 17, 9), voxel=0.11, origin=(-2.4, -0.4, 0.9), trunc=0.3), fx=ROOM_FX, cx=ROOM_CX,
                    frames=[(d, P, None)])
    if name == "boundary":
        # everything dyadic, identity pose, a plane at z = 2: the layer at z = 1 projects onto 8 i - 56.5 (pixel
        # boundaries, columns -0.5 and 15.5 among them) and the layer at z = 2.25 has sdf = -trunc exactly
        d = np.full((16, 16), 10000, np.uint16)
        return dict(volume=dict(dims=(16, 16, 12), voxel=0.125, origin=(-1.0625, -1.0625, 0.9375), trunc=0.25), fx=64.0, cx=7.5,
                    frames=[(d, np.eye(4), None)])
    if name in ("holes", "saturation"):
        d, P = room_frame(*ROOM_MOTIONS[1])
        vol = dict(dims=(40, 36, 44), voxel=0.1, origin=(-2.3, -1.9, 0.4), trunc=0.3)
        if name == "holes":
            rng = np.random.default_rng(19)
            d = np.where(rng.random(d.shape) < 0.3, 0, d).astype(np.uint16)
            return dict(volume=vol, fx=ROOM_FX, cx=ROOM_CX, frames=[(d, P, None)])
        return dict(volume=dict(vol, max_weight=2), fx=ROOM_FX, cx=ROOM_CX, frames=[(d, P, None)] * 4)
    if name in ("plane", "plane_edge"):
        # a fronto-parallel plane at z0 = 1.5, identity pose, dyadic voxel, origin and trunc (0.375 is no power of two:
        # sdf / trunc rounds); the volume is narrower than the view, so its last x and y layers are seen.  plane_edge:
        # the plane lies between the last two z layers
        d = np.full((48, 64), 7500, np.uint16)
        dz = 10 if name == "plane" else 7
        return dict(volume=dict(dims=(12, 10, dz), voxel=0.0625, origin=(-0.375, -0.3125, 1.125), trunc=0.375), fx=64.0, cx=31.5,
                    frames=[(d, np.eye(4), None)], z0=1.5)
    raise KeyError(name)


def hand_over(ctx, raycast=False, color=False):
    """The `plane` case fused on the context and handed over as its target: the surface list
    (icpk_tsdf_surface_to_target) or the ray cast from the frame's own pose (icpk_tsdf_raycast_to_target).  color: a
    volume with ICPK_TSDF_COLOR and a flat intensity of 0.5.  Returns the new target's size.  (For the lifetime tests
    of the features whose records speak of the target: a hand-over replaces it like any other new target.)"""
    from icp_slam_prototype_amd import binding

    c = case("plane")
    v = c["volume"]
    d, P, _ = c["frames"][0]
    ctx.tsdf_create(dims=v["dims"], voxel=v["voxel"], origin=v["origin"], trunc=v["trunc"],
                    flags=binding.TSDF_COLOR if color else 0)
    ctx.tsdf_integrate(d, P, np.full(d.shape, 0.5, np.float32) if color else None, fx=c["fx"], cx=c["cx"])
    if raycast:
        ctx.tsdf_raycast(P, shape=d.shape, fx=c["fx"], cx=c["cx"], z_near=0.25, z_far=3.0, step=0.1875, min_weight=1)
        ctx.tsdf_raycast_to_target()
    else:
        ctx.tsdf_extract_surface(1)
        ctx.tsdf_surface_to_target()
    assert ctx.target_size > 0
    return ctx.target_size


SMALL_CASES = ("room", "room_color", "odd", "boundary", "holes", "saturation", "plane", "plane_edge")


@functools.lru_cache(maxsize=None)
def model(name):
    """The model run over the case: dict(n_updated per frame, tsdf / weight / intensity after every frame, surface
    (min_weight 1) after the last, volume: the tsdf_model.Volume).  Arrays are read-only."""
    c = case(name)
    vol = tsdf_model.Volume(**c["volume"])
    out = dict(n_updated=[], tsdf=[], weight=[], intensity=[], volume=vol)
    for d, P, inten in c["frames"]:
        out["n_updated"].append(vol.integrate(d, P, c["fx"], c["cx"], inten))
        out["tsdf"].append(vol.tsdf.copy())
        out["weight"].append(vol.weight.copy())
        out["intensity"].append(None if vol.intensity is None else vol.intensity.copy())
    out["surface"] = vol.extract(1)
    for a in out["tsdf"] + out["weight"] + [x for x in out["intensity"] if x is not None] + \
            [v for v in out["surface"].values() if isinstance(v, np.ndarray)] + [vol.tsdf, vol.weight]:
        a.flags.writeable = False
    return out
