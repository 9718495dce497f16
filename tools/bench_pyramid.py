"""Timing of the depth pyramid (icpk_depth_pyramid_build, K24) and of coarse-to-fine model tracking: the median over
--reps calls after --warmup calls, each call bracketed by HIP events on the context's stream (as
tools/bench_bilateral.py).  Prints one JSON line and writes it to profiles/pyramid_bench.json.  One run on one box: the
figures say what a frame pays there, nothing is asserted anywhere.

One synthetic 640 x 480 frame of the room with sensor noise.
  build_pyramid_us             icpk_depth_pyramid_build, 3 levels, level 0 the frame as given: upload (614 KB), one kernel
  build_pyramid_smooth_us      the same with smooth = the bilateral defaults: upload, K22, one kernel
  bilateral_depth_image_us     icpk_bilateral_depth_image at the defaults (upload, K22, download) from the same run
  backproject_us               icpk_backproject of the same frame (upload, back-projection, the count)
  backproject_level_us[l]      icpk_depth_pyramid_backproject of level l of the resident pyramid: no upload
The tracker: the room of tests/tsdf_cases.py (120 x 160, the 64^3 volume), three frames fused at their true poses; one
ModelTracker.track call of the fourth frame from the third pose, the model put back before every call.  Host wall
time of the whole call next to the events' time, since a track call is mostly launches and host waits.
  track_plain_19_us            max_iterations = 19, max_nn_dist = 0.1
  track_pyramid_10_5_4_us      pyramid = (10, 5, 4), the same gate
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from icp_slam_prototype_amd import binding, depth, synth
from icp_slam_prototype_amd.tsdf import ModelTracker, TsdfVolume


def timed(ctx, fn, warmup, reps, before=None):
    """(median microseconds between the events, median microseconds of host wall time); before(): untimed set-up"""
    stream = torch.cuda.ExternalStream(int(ctx.stream), device=torch.device("cuda", 0))
    us, wall = [], []
    for k in range(warmup + reps):
        if before is not None:
            before()
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        t1 = time.perf_counter()
        if k >= warmup:
            us.append(1000.0 * e0.elapsed_time(e1))
            wall.append(1e6 * (t1 - t0))
    return float(np.median(us)), float(np.median(wall))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import tsdf_cases as tc

    rows, cols = 480, 640
    fx, cx = float(synth.FX), float(synth.CX)
    img = synth.render_room_depth(rows, cols, np.eye(3), np.zeros(3), fx, cx, 0.002, np.random.default_rng(7))
    out = {"frame": [rows, cols], "reps": a.reps, "warmup": a.warmup, "levels": 3, "note": "one run on one box",
           "backproject_level_us": {}}
    res = np.empty_like(img)
    p, b = depth.pyramid_params(levels=3), depth.bilateral_params()
    with binding.Context(0) as ctx:
        out["build_pyramid_us"] = timed(ctx, lambda: depth.build_pyramid(ctx, img, p), a.warmup, a.reps)[0]
        out["build_pyramid_smooth_us"] = timed(ctx, lambda: depth.build_pyramid(ctx, img, p, smooth=b), a.warmup, a.reps)[0]
        out["bilateral_depth_image_us"] = timed(ctx, lambda: depth.bilateral_depth_image(ctx, img, b, out=res), a.warmup, a.reps)[0]
        out["backproject_us"] = timed(ctx, lambda: ctx.backproject(img, fx=fx, cx=cx), a.warmup, a.reps)[0]
        depth.build_pyramid(ctx, img, p)
        for l in range(3):
            out["backproject_level_us"][str(l)] = timed(ctx, lambda: depth.backproject_level(ctx, l, fx=fx, cx=cx), a.warmup, a.reps)[0]
    # one track call
    c = tc.case("room")
    geom = {k: c["volume"][k] for k in ("dims", "voxel", "origin", "trunc")}
    d4, _ = tc.room_frame(*tc.ROOM_FOURTH)
    P3 = c["frames"][2][1]
    out["tracker_frame"] = list(tc.ROOM_SHAPE)
    with binding.Context(0) as ctx:
        vol = TsdfVolume(ctx, **geom, fx=c["fx"], cx=c["cx"])
        for d, P, _ in c["frames"]:
            vol.integrate(d, P)
        model = vol.planes()[:2]
        for key, extra in (("track_plain_19", dict(max_iterations=19)), ("track_pyramid_10_5_4", dict(pyramid=(10, 5, 4)))):
            state = {}

            def before():
                vol.set_planes(*model)
                state["t"] = ModelTracker(vol, pose=P3, step=0.125, max_nn_dist=0.1, **extra)
                state["t"].frames = 3

            out[key + "_us"], out[key + "_wall_us"] = timed(ctx, lambda: state["t"].track(d4), a.warmup, a.reps, before)
    line = json.dumps(out)
    print(line)
    prof = os.path.join(ROOT, "profiles")
    os.makedirs(prof, exist_ok=True)
    with open(os.path.join(prof, "pyramid_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
