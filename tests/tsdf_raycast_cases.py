"""The ray-cast cases (K20) shared by tests/test_tsdf_raycast_host.py and tests/test_gpu_tsdf_raycast.py: a volume of
tsdf_cases, a view, and the counts the rule gives there.  Every model run is computed once per process and handed out
read-only."""
import functools

import numpy as np

import tsdf_cases as tc
import tsdf_raycast_model as rm

ROOM_VIEW = dict(shape=tc.ROOM_SHAPE, fx=tc.ROOM_FX, cx=tc.ROOM_CX, z_near=0.25, z_far=6.0, step=0.125, min_weight=1)
PLANE_VIEW = dict(shape=(48, 64), fx=64.0, cx=31.5, z_near=0.25, z_far=3.0, step=0.1875, min_weight=1)

# name -> (case of tsdf_cases, pose, view, crossings, listed)
VIEWS = {
    "room": ("room", lambda: tc.pose(*tc.ROOM_FOURTH), ROOM_VIEW, 13889, 13126),
    "room_min_weight_2": ("room", lambda: tc.pose(*tc.ROOM_FOURTH), dict(ROOM_VIEW, min_weight=2), 12544, 11568),
    "room_z_far": ("room", lambda: tc.pose(*tc.ROOM_FOURTH), dict(ROOM_VIEW, z_far=2.5), 2256, 2079),
    "plane": ("plane", lambda: np.eye(4), PLANE_VIEW, 672, 432),
    "plane_reversed": ("plane", lambda: tc.pose((0, 180, 0), (0, 0, 1.6)), dict(PLANE_VIEW, z_near=0.01, step=0.03), 0, 0),
    # 37 x 53: a multiple of neither the 8 x 8 / 16 x 16 tile nor the 256-pixel chunk
    "odd": ("odd", lambda: tc.case("odd")["frames"][0][1], dict(shape=(37, 53), fx=40.0, cx=26.0, z_near=0.1, z_far=4.0,
                                                                 step=0.15, min_weight=1), 322, 169),
    "holes": ("holes", lambda: tc.case("holes")["frames"][0][1], dict(ROOM_VIEW, step=0.15), 204, 0),
    # (not in the table: the intensity plane)
    "room_color": ("room_color", lambda: tc.pose(*tc.ROOM_FOURTH), ROOM_VIEW, None, None),
}
TABLE = ("room", "room_min_weight_2", "room_z_far", "plane", "plane_reversed", "odd", "holes")


def view(name):
    """(case name, pose (4, 4) float64, view keywords)"""
    case, pose, v, _, _ = VIEWS[name]
    return case, np.asarray(pose(), np.float64), v


@functools.lru_cache(maxsize=None)
def model(name):
    """tsdf_raycast_model.raycast with its debug output over the view; arrays are read-only"""
    case, P, v = view(name)
    out = rm.raycast(tc.model(case)["volume"], P, debug=True, **v)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return out


def volume_params(binding, case):
    v = tc.case(case)["volume"]
    return binding.tsdf_params(dims=v["dims"], voxel=v["voxel"], origin=v["origin"], trunc=v["trunc"],
                               max_weight=v.get("max_weight"), flags=binding.TSDF_COLOR if v.get("color") else 0)


def ray_params(binding, v):
    return binding.tsdf_raycast_params(**v)
