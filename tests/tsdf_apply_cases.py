"""The cases of the signed update rule (K30) shared by tests/test_tsdf_apply_host.py and the GPU tests: volumes, the
frames of a call and its op list, over the shapes of tests/tsdf_cases.py.  Every model run is computed once per process
and handed out read-only."""
import functools

import tsdf_apply_model
import tsdf_cases as tc
import tsdf_model

P, M = +1, -1

# a camera at the origin turned right round: every voxel of every volume here lies behind it
BEHIND = tc.pose((0.0, 180.0, 0.0), (0.0, 0.0, 0.0))


def drift(pose, rot_deg, shift):
    """the pose with a small error composed onto it: where a tracker that drifts would have fused the frame"""
    return pose @ tc.pose(rot_deg, shift)


def _single(name):
    """one of K19's shapes: its one frame in, at a drifted pose too, and out again in another order"""
    c = tc.case(name)
    d, pose, _ = c["frames"][0]
    off = drift(pose, (1.0, -2.0, 0.5), (0.03, -0.02, 0.04))
    ops = [(M, 0, pose), (P, 0, pose), (P, 0, off), (P, 0, pose), (M, 0, off), (M, 0, pose)]
    return dict(volume=c["volume"], fx=c["fx"], cx=c["cx"], frames=[d], intensities=None, ops=ops)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(volume (keywords of tsdf_model.Volume), fx, cx, frames: depth images, intensities: as many or None, ops: list
    of (sign, frame, pose))"""
    if name in ("odd", "boundary", "holes"):
        return _single(name)
    if name == "saturation":
        # max_weight 2: + up to the cap and past it, then - until nothing is left and once more (that one writes
        # nothing), then two in and one out again so that the end is not the fresh volume
        c = tc.case(name)
        d, pose, _ = c["frames"][0]
        return dict(volume=c["volume"], fx=c["fx"], cx=c["cx"], frames=[d], intensities=None,
                    ops=[(P, 0, pose)] * 4 + [(M, 0, pose)] * 3 + [(P, 0, pose), (P, 0, pose), (M, 0, pose)])
    if name in ("tiny", "tail"):
        # tiny: 5 x 3 x 7 = 105 voxels around the sphere and the back wall, less than one workgroup; tail: 19 x 9 x 3 =
        # 513 = 2 * 256 + 1 voxels, the last chunk holds one
        (d0, p0), (d1, p1) = tc.room_frame(*tc.ROOM_MOTIONS[0]), tc.room_frame(*tc.ROOM_MOTIONS[1])
        vol = dict(dims=(5, 3, 7), voxel=0.3, origin=(-0.4, 0.0, 1.6), trunc=0.6) if name == "tiny" else \
            dict(dims=(19, 9, 3), voxel=0.12, origin=(-0.8, -0.2, 3.3), trunc=0.3)
        ops = [(P, 0, p0), (P, 1, p1), (M, 0, p0), (P, 1, drift(p1, (0.0, 2.0, 0.0), (0.05, 0.0, 0.0))), (M, 1, p1)]
        return dict(volume=vol, fx=tc.ROOM_FX, cx=tc.ROOM_CX, frames=[d0, d1], intensities=None, ops=ops)
    if name in ("room", "room_color"):
        # 64^3, 16 ops over 2 frames: - on the fresh volume, a frame in at a wrong pose and out again, the same frame
        # removed twice, a pose with every voxel behind the camera with either sign
        c = tc.case(name)
        (d0, p0, i0), (d1, p1, i1) = c["frames"][0], c["frames"][1]
        q0, q1 = drift(p0, (2.0, -3.0, 1.0), (0.05, 0.02, -0.04)), drift(p1, (-1.0, 2.0, 0.0), (-0.03, 0.04, 0.02))
        ops = [(M, 0, p0), (P, 0, p0), (P, 1, p1), (P, 0, q0), (M, 0, q0), (M, 1, p1), (M, 1, p1), (P, 1, BEHIND),
               (P, 1, p1), (P, 0, p0), (M, 0, p0), (P, 1, q1), (M, 1, q1), (P, 0, p0), (M, 0, BEHIND), (P, 1, p1)]
        return dict(volume=c["volume"], fx=c["fx"], cx=c["cx"], frames=[d0, d1],
                    intensities=[i0, i1] if name == "room_color" else None, ops=ops)
    if name == "room_capped":
        # the 64^3 room with max_weight 3, every chunk of it: + up to the cap and past it, then - (from the cap: no
        # inverse any more), down to nothing on the voxels one frame alone saw, and in again
        c = tc.case("room")
        (d0, p0, _), (d1, p1, _) = c["frames"][0], c["frames"][1]
        ops = [(P, 0, p0), (P, 1, p1), (P, 0, p0), (P, 1, p1), (P, 0, p0), (M, 0, p0), (M, 1, p1), (M, 0, p0), (M, 0, p0),
               (P, 1, p1), (M, 1, p1), (M, 1, p1), (P, 0, p0)]
        return dict(volume=dict(c["volume"], max_weight=3), fx=c["fx"], cx=c["cx"], frames=[d0, d1], intensities=None, ops=ops)
    if name == "fresh_minus":
        # nothing but removals from a fresh volume: nothing is written
        c = tc.case("room")
        (d0, p0, _), (d1, p1, _) = c["frames"][0], c["frames"][1]
        return dict(volume=c["volume"], fx=c["fx"], cx=c["cx"], frames=[d0, d1], intensities=None,
                    ops=[(M, 0, p0), (M, 1, p1), (M, 0, p0)])
    if name in ("abcb", "ac"):
        # the room's three frames in and the second out again, and the first and the third alone: the removal test.
        # trunc is no power of two here: with the room's 0.25 every sample is a multiple of 2^-20, every sum is exact and
        # the removal lands on +A +C bit for bit, which measures nothing
        c = tc.case("room")
        frames = [f[0] for f in c["frames"]]
        pa, pb, pc = (f[1] for f in c["frames"])
        ops = [(P, 0, pa), (P, 1, pb), (P, 2, pc), (M, 1, pb)]
        if name == "ac":  # (a call carries no more frames than ops)
            frames, ops = [frames[0], frames[2]], [(P, 0, pa), (P, 1, pc)]
        return dict(volume=dict(c["volume"], trunc=0.3), fx=c["fx"], cx=c["cx"], frames=frames, intensities=None, ops=ops)
    raise KeyError(name)


BYTE_CASES = ("tiny", "tail", "odd", "boundary", "holes", "saturation", "room", "room_color", "room_capped", "fresh_minus", "abcb", "ac")

# the removal test: +A +B +C -B against +A +C.  A voxel is hit by some of A, B, C: the worst tsdf_apply_model.error_bound
# over the eight subsets on either side (11 EPS, for a voxel B and another frame hit, and 2.5 EPS for +A +C), added
REMOVAL_BOUND = (tsdf_apply_model.worst_error_bound([(P, "a"), (P, "b"), (P, "c"), (M, "b")]) +
                 tsdf_apply_model.worst_error_bound([(P, "a"), (P, "c")])) * tsdf_apply_model.EPS


def fresh(name):
    """a fresh tsdf_model.Volume of the case's shape"""
    return tsdf_model.Volume(**case(name)["volume"])


@functools.lru_cache(maxsize=None)
def model(name):
    """The model run over the case from a fresh volume: dict(counts, tsdf, weight, intensity or None).  Read-only."""
    c = case(name)
    vol = fresh(name)
    counts = tsdf_apply_model.apply(vol, c["frames"], c["ops"], c["fx"], c["cx"], c["intensities"])
    out = dict(counts=counts, tsdf=vol.tsdf, weight=vol.weight, intensity=vol.intensity)
    for a in (vol.tsdf, vol.weight, vol.intensity):
        if a is not None:
            a.flags.writeable = False
    return out
