#!/usr/bin/env python
"""Diagnostic: what tracking against the distance field itself (K29) costs next to tracking against a ray cast of it.

Medians of 20 calls after 3, on the room scene at 120 x 160 and 480 x 640, HIP events on the context's stream and wall
time around the same call:
  - icpk_align_sdf alone, per level of a three-level pyramid with the tracker's iteration counts (10, 5, 4): two
    launches per iteration, one copy and one wait per call;
  - one tsdf.ModelTracker(sdf=True, pyramid=(10, 5, 4)).track call -- the pyramid build, three sdf loops and the
    integration of the frame; no ray cast;
  - on the same frames, tsdf.ModelTracker(projective=True, pyramid=(10, 5, 4)).track -- the pyramid build, per level a
    ray cast and a projective loop, and the integration of the frame.
Every timed call aligns the same second frame to the same model (the trackers' state is put back before each call).
Nothing is asserted; one run on one box says what the order of magnitude is, not more.

    python tools/bench_sdf_track.py [--reps 20] [--warmup 3] [--out profiles/sdf_track_bench.json]
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
from icp_slam_prototype_amd.tsdf import ModelTracker, TsdfVolume  # noqa: E402

COUNTS = (10, 5, 4)
GEOM = {k: tc.ROOM_VOLUME[k] for k in ("dims", "voxel", "origin", "trunc")}


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


def error_mm(pose, truth):
    return round(1000.0 * float(np.linalg.norm((np.linalg.inv(truth) @ pose)[:3, 3])), 3)


def measure(shape, reps, warmup):
    fx, cx, frames = frames_at(shape)
    (d0, P0), (d1, P1) = frames
    rec = {"shape": list(shape), "fx": fx, "cx": cx}
    with binding.Context(0) as ctx:
        vol = TsdfVolume(ctx, **GEOM, fx=fx, cx=cx)
        tracker = ModelTracker(vol, pose=P0, sdf=True, pyramid=COUNTS)
        tracker.track(d0)
        model = vol.planes()[:2]
        depth.build_pyramid(ctx, d1, depth.pyramid_params(levels=len(COUNTS)))
        for l in range(len(COUNTS) - 1, -1, -1):
            p = binding.default_sdf_params(level=l, fx=fx, cx=cx, max_iterations=COUNTS[l])
            rec[f"align_sdf_level{l}_{COUNTS[l]}_iterations"] = timed(ctx, lambda: binding.align_sdf(ctx, P0, p), reps, warmup)
            rec[f"accepted_level{l}"] = binding.sdf_reduce(ctx, P0, p)[1]

        def rewind():
            vol.set_planes(*model)
            tracker.pose, tracker.frames = P0.copy(), 1

        rec["model_tracker_sdf_track"] = timed(ctx, lambda: tracker.track(d1), reps, warmup, before=rewind)
        rec["model_tracker_sdf_error_mm"] = error_mm(tracker.pose, P1)
    with binding.Context(0) as ctx:
        vol = TsdfVolume(ctx, **GEOM, fx=fx, cx=cx)
        tracker = ModelTracker(vol, pose=P0, step=0.125, projective=True, pyramid=COUNTS)
        tracker.track(d0)
        model = vol.planes()[:2]

        def rewind_model():
            vol.set_planes(*model)
            tracker.pose, tracker.frames = P0.copy(), 1

        rec["model_tracker_projective_track"] = timed(ctx, lambda: tracker.track(d1), reps, warmup, before=rewind_model)
        rec["model_tracker_projective_error_mm"] = error_mm(tracker.pose, P1)
    for k in ("device_ms", "wall_ms"):
        rec[f"sdf_over_projective_{k}"] = round(rec["model_tracker_sdf_track"][k] / rec["model_tracker_projective_track"][k], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdf_track_bench.json"))
    a = ap.parse_args()
    out = {"command": f"python tools/bench_sdf_track.py --reps {a.reps} --warmup {a.warmup}",
           "note": "medians; one run on one MI355X: an order of magnitude, not a comparison to rely on",
           "pyramid": list(COUNTS), "sizes": [measure(shape, a.reps, a.warmup) for shape in ((120, 160), (480, 640))]}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
