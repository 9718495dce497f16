#!/usr/bin/env python
"""Diagnostic: what the frame view (K28) costs, and projective frame-to-frame odometry next to frame-to-model tracking.

Medians of 20 calls after 3, on the room scene at 120 x 160 and 480 x 640, HIP events on the context's stream and wall
time around the same call:
  - icpk_frame_view_build alone (three levels, one launch, no count asked for: the wall time is the enqueue, the
    device time the two kernels);
  - one odometry.ProjectiveOdometry.track call (pyramid (10, 5, 4): the pyramid build, three projective loops, the
    view's rebuild with its counts);
  - on the same frames, tsdf.ModelTracker(projective=True, pyramid=(10, 5, 4)).track -- the pyramid build, per level a
    ray cast and a projective loop, and the integration of the frame.
Every timed call aligns the same second frame to the same first one (the trackers' state is put back before each
call).  Nothing is asserted; one run on one box says what the order of magnitude is, not more.

    python tools/bench_frame_odometry.py [--reps 20] [--warmup 3] [--out profiles/frame_view_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # (before the library: both bring a HIP runtime, and torch's must be the first initialised)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tsdf_cases as tc  # noqa: E402
from icp_slam_prototype_amd import binding, depth  # noqa: E402
from icp_slam_prototype_amd.odometry import ProjectiveOdometry  # noqa: E402
from icp_slam_prototype_amd.tsdf import ModelTracker, TsdfVolume  # noqa: E402

COUNTS = (10, 5, 4)


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def frames_at(shape):
    """the room's third and fourth frame at `shape`, the field of view kept: (fx, cx, [(depth, pose)] x 2)"""
    fx, cx = tc.ROOM_FX * shape[1] / tc.ROOM_SHAPE[1], tc.ROOM_CX * shape[1] / tc.ROOM_SHAPE[1]
    return fx, cx, [tc.room_frame(*m, shape=shape, fx=fx, cx=cx) for m in (tc.ROOM_MOTIONS[2], tc.ROOM_FOURTH)]


def timed(ctx, fn, reps, warmup, before=None):
    stream = torch.cuda.ExternalStream(int(ctx.stream), device=torch.device("cuda", 0))
    dev, wall = [], []
    for k in range(warmup + reps):
        if before is not None:
            before()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        dt = time.perf_counter() - t0
        if k >= warmup:
            dev.append(e0.elapsed_time(e1))
            wall.append(1000.0 * dt)
    return dict(device_ms=round(median(dev), 4), wall_ms=round(median(wall), 4))


def measure(shape, reps, warmup):
    fx, cx, frames = frames_at(shape)
    (d0, P0), (d1, P1) = frames
    rec = {"shape": list(shape), "fx": fx, "cx": cx}
    with binding.Context(0) as ctx:
        depth.build_pyramid(ctx, d0, depth.pyramid_params(levels=len(COUNTS)))
        rec["frame_view_build"] = timed(ctx, lambda: binding.frame_view_build(ctx, P0, fx=fx, cx=cx, counts=False), reps, warmup)
        rec["frame_view_build_with_counts"] = timed(ctx, lambda: binding.frame_view_build(ctx, P0, fx=fx, cx=cx), reps, warmup)
        rec["n_valid"], rec["n_no_normal"] = binding.frame_view_build(ctx, P0, fx=fx, cx=cx)
        odo = ProjectiveOdometry(ctx, pose=P0, pyramid=COUNTS, fx=fx, cx=cx)
        odo.track(d0)

        def rewind():
            # the view of frame 0 at its pose again: every timed call aligns frame 1 to frame 0
            depth.build_pyramid(ctx, d0, odo.pyramid_params)
            odo.pose = P0.copy()
            odo._build_view()

        rec["projective_odometry_track"] = timed(ctx, lambda: odo.track(d1), reps, warmup, before=rewind)
        E = np.linalg.inv(P1) @ odo.pose
        rec["odometry_error_mm"] = round(1000.0 * float(np.linalg.norm(E[:3, 3])), 3)
    with binding.Context(0) as ctx:
        vol = TsdfVolume(ctx, **{k: tc.ROOM_VOLUME[k] for k in ("dims", "voxel", "origin", "trunc")}, fx=fx, cx=cx)
        tracker = ModelTracker(vol, pose=P0, step=0.125, projective=True, pyramid=COUNTS)
        tracker.track(d0)
        model = vol.planes()[:2]

        def rewind_model():
            vol.set_planes(*model)
            tracker.pose, tracker.frames = P0.copy(), 1

        rec["model_tracker_projective_track"] = timed(ctx, lambda: tracker.track(d1), reps, warmup, before=rewind_model)
        E = np.linalg.inv(P1) @ tracker.pose
        rec["model_tracker_error_mm"] = round(1000.0 * float(np.linalg.norm(E[:3, 3])), 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_view_bench.json"))
    a = ap.parse_args()
    out = {"command": f"python tools/bench_frame_odometry.py --reps {a.reps} --warmup {a.warmup}",
           "note": "medians; one run on one MI355X: an order of magnitude, not a comparison to rely on",
           "pyramid": list(COUNTS), "sizes": [measure(shape, a.reps, a.warmup) for shape in ((120, 160), (480, 640))]}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
