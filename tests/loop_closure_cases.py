"""The loop of tests/test_gpu_loop_closure.py: the room at 120 x 160, the camera out along an arc and back to near the
start, thirteen frames; the poses a drifting tracker would hand over -- every step of the truth followed by one fixed
small error, so that the error accumulates to about K28's s = 1 row (6 deg / 83 mm) at the revisit --; and the fern
part of the rehearsal, which needs no GPU (icpk_fern_encode_host over depth.pyramid_host)."""
import functools

import numpy as np

import tsdf_cases as tc
from icp_slam_prototype_amd import binding, depth

YAW = (0.0, 3.0, 6.0, 9.0, 12.0, 15.0, 18.0, 14.5, 11.5, 8.5, 5.5, 2.5, 0.5)  # degrees about y: out and back
STEP_DRIFT = ((0.0, 0.5, 0.0), (0.007, 0.0, 0.0))  # composed onto every step: 12 steps make 6 deg / 84 mm
LEVELS = 3
# the knobs, from fern_rehearsal(): with the default harvest_above (51 of 256 ferns) only frames 0 and 3 are harvested --
# two nodes, no loop --; a 3 degree step changes 18 .. 21 ferns, so 15 harvests every outbound frame (7 keyframes), and
# the frames on the way back, half a degree off an outbound one, differ from it in at most 8
FERN = dict(harvest_above=15)
MAX_DISS = 12
MIN_GAP = 4


def motion(k):
    return (0.0, YAW[k], 0.0), (0.012 * YAW[k], 0.0, 0.0)


@functools.lru_cache(maxsize=None)
def loop():
    """dict(depths, truth, given): the frames, their true poses and the drifting ones"""
    frames = [tc.room_frame(*motion(k)) for k in range(len(YAW))]
    truth = [f[1] for f in frames]
    D = tc.pose(*STEP_DRIFT)
    given = [truth[0].copy()]
    for k in range(1, len(truth)):
        given.append(given[-1] @ np.linalg.inv(truth[k - 1]) @ truth[k] @ D)
    return dict(depths=[f[0] for f in frames], truth=truth, given=given)


def pose_error(a, b):
    """(degrees, metres) between two poses"""
    E = np.linalg.inv(a) @ b
    return float(np.degrees(np.arccos(np.clip((np.trace(E[:3, :3]) - 1) / 2, -1, 1)))), float(np.linalg.norm(E[:3, 3]))


@functools.lru_cache(maxsize=None)
def fern_rehearsal():
    """The harvest and the search of K27 replayed on the host over the loop's frames with FERN at the
    coarsest level: dict(keyframes: the frames harvested, rows: per frame (nearest keyframe's frame, its diss,
    harvested), harvest_above)"""
    p = binding.default_fern_params(level=LEVELS - 1, **FERN)
    codes = [binding.fern_encode_host(p, depth.pyramid_host(d, LEVELS - 1, depth.pyramid_params(levels=LEVELS)))[0]
             for d in loop()["depths"]]
    keyframes, rows = [], []
    for k, code in enumerate(codes):
        diss = [binding.fern_dissimilarity_host(code, codes[j], p.n_ferns) for j in keyframes]
        best = int(np.argmin(diss)) if diss else -1
        harvested = not diss or min(diss) > p.harvest_above
        rows.append((keyframes[best] if diss else -1, diss[best] if diss else -1, harvested,
                     sorted(zip(diss, keyframes))[:3]))
        if harvested:
            keyframes.append(k)
    return dict(keyframes=keyframes, rows=rows, harvest_above=int(p.harvest_above), n_ferns=int(p.n_ferns))
