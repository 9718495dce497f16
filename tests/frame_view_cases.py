"""The small cases of the frame view rule (K28) shared by tests/test_frame_view_host.py, tests/test_gpu_frame_view.py and
the thread test: a level-0 depth frame (with or without intensities), the LEVEL-0 intrinsics, the number of pyramid
levels and a pose.  Every model run is computed once per process and handed out read-only."""
import functools

import numpy as np

import frame_view_model as fm
import projective_color_model as qm
import projective_model as jm
import pyramid_model as pm
import tsdf_cases as tc

ROOM_POSE = lambda: tc.pose(*tc.ROOM_MOTIONS[2])  # frame 3 of the room at its true pose


def _hole_5x7():
    img = (6000 + 40 * np.arange(5)[:, None] + 25 * np.arange(7)[None, :]).astype(np.uint16)
    img[2, 4] = 0  # beside the centre (2, 3)
    return img


def _edge_on():
    """Pixel (3, 1) of a 5 x 3 image whose normal is EXACTLY perpendicular to its ray.  cx = -2^25, where floats are 4
    apart: the columns 0, 1, 2 all round to -cx (the east and west neighbours lie on the pixel's own ray) while the rows
    2 and 4 round to different values, so with fx = 2^25 the cross product is (-g, 0, g) exactly, the vertex is
    (v_z, v_y, v_z), and the dot is fl(-g' v_z + 0) + g' v_z = 0."""
    img = np.full((5, 3), 5000, np.uint16)
    img[3, 2], img[3, 0], img[4, 1], img[2, 1], img[3, 1] = 9000, 6000, 7000, 5500, 6500
    return img


def _room3():
    return tc.case("room")["frames"][2][0]


def _room3_intensity():
    return tc.room_intensity(*tc.ROOM_MOTIONS[2])


IDENTITY = lambda: np.eye(4)
TILT = lambda: tc.pose((3.0, -5.0, 2.0), (0.1, -0.2, 0.3))

# name -> dict(frame: the level-0 depth image, fx, cx: its LEVEL-0 intrinsics, levels, pose, intensity (optional))
CASES = {
    "1x1": dict(frame=lambda: np.array([[7500]], np.uint16), fx=64.0, cx=0.0, levels=1, pose=TILT),
    # one interior pixel
    "3x3": dict(frame=lambda: (5000 + 100 * np.arange(9).reshape(3, 3)).astype(np.uint16), fx=8.0, cx=1.0, levels=1, pose=TILT),
    # a hole beside the centre: its four neighbours lose their normal
    "5x7_hole": dict(frame=_hole_5x7, fx=16.0, cx=3.0, levels=1, pose=TILT),
    # a fronto-parallel plane at the identity
    "plane": dict(frame=lambda: np.full((9, 11), 7500, np.uint16), fx=16.0, cx=5.0, levels=1, pose=IDENTITY),
    # s . v == 0 exactly at pixel (3, 1)
    "edge_on": dict(frame=_edge_on, fx=2.0 ** 25, cx=-(2.0 ** 25), levels=1, pose=IDENTITY),
    # the room's frame 3 at its true pose: 120 x 160, 60 x 80, 30 x 40 -- 75 + 19 + 5 workgroups in one launch
    "room": dict(frame=_room3, fx=tc.ROOM_FX, cx=tc.ROOM_CX, levels=3, pose=ROOM_POSE),
    # ... with its intensities beside the pyramid
    "room_color": dict(frame=_room3, fx=tc.ROOM_FX, cx=tc.ROOM_CX, levels=3, pose=ROOM_POSE, intensity=_room3_intensity),
}
NAMES = tuple(CASES)
ROOM_LEVELS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(depth: the level-0 frame, intensity (or None), images / intensities: the pyramid's levels, fx, cx, levels,
    pose (4, 4))"""
    c = CASES[name]
    depth = np.ascontiguousarray(c["frame"](), np.uint16)
    images = pm.pyramid(depth, c["levels"])
    inten = np.ascontiguousarray(c["intensity"](), np.float32) if "intensity" in c else None
    intens = None if inten is None else qm.intensity_pyramid(depth, inten, c["levels"])
    for a in [depth] + list(images) + ([] if inten is None else [inten] + list(intens)):
        a.setflags(write=False)
    return dict(depth=depth, intensity=inten, images=images, intensities=intens, fx=c["fx"], cx=c["cx"], levels=c["levels"],
                pose=np.asarray(c["pose"](), np.float64))


def level_camera(name, level):
    """(fx_l, cx_l) float32: the LEVEL's own intrinsics"""
    c = case(name)
    scale = np.float32(2 ** level)
    return np.float32(c["fx"]) / scale, np.float32(c["cx"]) / scale


@functools.lru_cache(maxsize=None)
def expected(name, level):
    """The model's view of a level: dict(planes, n_valid, n_no_normal, listed); arrays are read-only."""
    c = case(name)
    fx_l, cx_l = level_camera(name, level)
    out = fm.view(c["images"][level], fx_l, cx_l, c["pose"], None if c["intensities"] is None else c["intensities"][level])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def self_pairs(name, level, pose=None):
    """THE PROJECTIVE RULE (the numpy model) for the level against its own view at E == P: the model's pixel and dist"""
    c = case(name)
    fx_l, cx_l = level_camera(name, level)
    P = c["pose"] if pose is None else pose
    img = c["images"][level]
    planes = expected(name, level)["planes"] if pose is None else fm.view(img, fx_l, cx_l, P)["planes"]
    return jm.pixels(img, fx_l, cx_l, planes, img.shape, fx_l, cx_l, P, P)


def check_conditions():
    """What the cases are for, asserted on the model's output."""
    e = expected("1x1", 0)
    assert (e["n_valid"], e["n_no_normal"]) == (0, 1) and not e["planes"].any()
    e = expected("3x3", 0)
    assert (e["n_valid"], e["n_no_normal"]) == (1, 8) and e["listed"][1, 1]
    e = expected("5x7_hole", 0)
    # the interior is 3 x 5; the hole and its four neighbours drop out of it
    assert e["n_valid"] == 15 - 5 and e["n_no_normal"] == 35 - 1 - 10
    for r, c in ((2, 3), (1, 4), (3, 4), (2, 5), (2, 4)):
        assert not e["listed"][r, c] and not e["planes"][:, r, c].any()
    e = expected("plane", 0)
    lst = e["listed"]
    assert e["n_valid"] == 7 * 9 and (e["planes"][3][lst] == 0).all() and (e["planes"][4][lst] == 0).all()
    assert (e["planes"][5][lst] == -1).all() and (e["planes"][2][lst] == np.float32(7500) / np.float32(5000)).all()
    assert (e["planes"][6][lst] == np.float32(7500) / np.float32(5000)).all()
    # the dot of the edge-on pixel is exactly 0, its normal exists and is NOT negated
    c = case("edge_on")
    fx_l, cx_l = level_camera("edge_on", 0)
    has, s = jm.cross_normals(c["images"][0], fx_l, cx_l)
    F = np.float32
    vz = F(c["images"][0][3, 1]) / F(5000)
    vx, vy = (F(1) - cx_l) * vz / fx_l, (F(3) - cx_l) * vz / fx_l
    assert has[3, 1] and (s[0][3, 1] * vx + s[1][3, 1] * vy) + s[2][3, 1] * vz == 0
    e = expected("edge_on", 0)
    assert e["listed"][3, 1] and e["planes"][5, 3, 1] == s[2][3, 1] > 0
    # the room: every level lists most of its pixels, the border is among those without a normal
    for l in ROOM_LEVELS:
        e = expected("room", l)
        rows, cols = case("room")["images"][l].shape
        assert e["n_valid"] > rows * cols // 2 and e["n_no_normal"] >= 2 * (rows + cols) - 4
    assert expected("room_color", 0)["planes"][7].any() and not expected("room", 0)["planes"][7].any()


def device_setup(ctx, name, depth_front):
    """The case on a context: the frame's pyramid built (with its intensities).  No volume is made."""
    c = case(name)
    return depth_front.build_pyramid(ctx, c["depth"], depth_front.pyramid_params(levels=c["levels"]), intensity=c["intensity"])


# ---- the loop through the frame view: the room's fourth frame against the view of frame 3 -----------------------------
GRADIENT_RADIUS = 0.1  # metres at level 0; level l takes 2^l times it


@functools.lru_cache(maxsize=None)
def next_frame():
    """the room's fourth frame: dict(depth, intensity, images, intensities (3 levels), truth: its true pose)"""
    depth, truth = tc.room_frame(*tc.ROOM_FOURTH)
    depth = np.ascontiguousarray(depth, np.uint16)
    inten = np.ascontiguousarray(tc.room_intensity(*tc.ROOM_FOURTH), np.float32)
    images, intens = pm.pyramid(depth, 3), qm.intensity_pyramid(depth, inten, 3)
    for a in [depth, inten] + list(images) + list(intens):
        a.setflags(write=False)
    return dict(depth=depth, intensity=inten, images=images, intensities=intens, truth=truth)


@functools.lru_cache(maxsize=None)
def view_gradients(level):
    """THE VIEW GRADIENT RULE (the numpy model) over the planes of a level of room_color's view: (3, rows, cols)"""
    g = qm.view_gradients(expected("room_color", level)["planes"], GRADIENT_RADIUS * 2 ** level)[0]
    g.setflags(write=False)
    return g


def loop_args(level, pose=None, color=False):
    """the arguments of projective_model.pixels (color: of projective_color_model.pixels) for level `level` of the fourth
    frame against the same level of the view of frame 3; pose: default the view's own"""
    name = "room_color" if color else "room"
    f, c = next_frame(), case(name)
    fx_l, cx_l = level_camera(name, level)
    img = f["images"][level]
    out = dict(level=img, fx_s=fx_l, cx_s=cx_l, view=expected(name, level)["planes"], view_shape=img.shape, fx_v=fx_l, cx_v=cx_l,
               view_pose=c["pose"], pose=c["pose"] if pose is None else pose)
    if color:
        out.update(level_intensity=f["intensities"][level], gradient=view_gradients(level))
    return out
