"""The cases of the moving volume (K23) shared by tests/test_tsdf_shift_host.py and tests/test_gpu_tsdf_shift.py: the
shifts every small case is put through, and a walk along x through a volume narrower than the walk, run once on the
numpy models."""
import functools

import numpy as np

import tsdf_cases as tc
import tsdf_model
import tsdf_shift_model as sm

CASES = ("room", "room_color", "odd")


def named_shifts(dims):
    return [(3, -2, 1), (-1, 0, 0), (1, 0, 0), (0, 0, -4), (4, 4, 4), (-2, 3, -1), (0, 0, 0), (dims[0], 0, 0),
            (0, -dims[1] - 5, 0)]


def all_shifts(dims):
    """the named shifts, then s_x = -5 .. 5 alone (every misalignment of a four-word load along x, both signs) and with
    s_y = 1, s_z = -1"""
    return named_shifts(dims) + [(sx, 0, 0) for sx in range(-5, 6)] + [(sx, 1, -1) for sx in range(-5, 6)]


WALK_VOLUME = dict(dims=(32, 64, 64), voxel=0.0625, origin=(-1.0, -1.9, 0.4), trunc=0.25)
WALK_STEPS, WALK_STEP, WALK_EVERY = 16, 0.125, 2


@functools.lru_cache(maxsize=None)
def walk_frames():
    return [tc.room_frame((0.0, 0.0, 0.0), (WALK_STEP * n, 0.0, 0.0)) for n in range(WALK_STEPS)]


@functools.lru_cache(maxsize=None)
def walk_model():
    """TsdfVolume.follow(pose, every=2) in front of every integration, on the models: dict(volume (after the walk),
    streamed (one leaving list per shift, empty ones included), shifts, final (the last surface list), n_updated)"""
    vol = tsdf_model.Volume(**WALK_VOLUME)
    voxel = np.float64(vol.voxel)
    ref, streamed, shifts, updated = None, [], [], []
    for d, P in walk_frames():
        c = P[:3, 3].astype(np.float64)
        if ref is None:
            ref = c.copy()
        k = sm.follow_steps(c, ref, voxel)
        if (np.abs(k) >= WALK_EVERY).any():
            streamed.append(sm.leaving(vol, k, 1))
            vol = sm.shifted(vol, k)
            shifts.append(tuple(int(x) for x in k))
            ref = ref + k.astype(np.float64) * voxel
        updated.append(vol.integrate(d, P, tc.ROOM_FX, tc.ROOM_CX))
    return dict(volume=vol, streamed=streamed, shifts=shifts, final=vol.extract(1), n_updated=updated)


def walk_union(streamed, final):
    """all points of the streamed lists and the final list, (3, n)"""
    return np.concatenate([s["points"] for s in streamed] + [final["points"]], axis=1)
