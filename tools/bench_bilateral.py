"""Timing of the bilateral filter of a depth frame (icpk_bilateral_depth_image, K22): the median over --reps calls after
--warmup calls, each call bracketed by HIP events on the context's stream (as tools/bench_tsdf_raycast.py).  Prints one
JSON line and writes it to profiles/bilateral_bench.json.

One synthetic 640 x 480 frame of the room with sensor noise.  Every call uploads the frame, runs one kernel and brings
the result back: 614 KB each way, whatever the filter.
  filter_depth_image_us        K6 (icpk_filter_depth_image: range clamp + 5 x 5 close) on the same image in the same run:
                               the yardstick, since it moves the same bytes and does far less arithmetic per pixel
  bilateral_us[radius]         icpk_bilateral_depth_image at radius 1, 3 and 6 (9, 49 and 169 taps), sigma_space = radius / 1.5,
                               sigma_range 30
  backproject_smoothed_us      icpk_backproject_smoothed at the defaults: upload, filter, back-projection, the count
  backproject_us               icpk_backproject of the same frame: the same without the filter
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from icp_slam_prototype_amd import binding, depth, synth


def timed(ctx, fn, warmup, reps):
    stream = torch.cuda.ExternalStream(int(ctx.stream), device=torch.device("cuda", 0))
    for _ in range(warmup):
        fn()
    us = []
    for _ in range(reps):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        us.append(1000.0 * e0.elapsed_time(e1))
    return float(np.median(us))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    rows, cols = 480, 640
    fx, cx = float(synth.FX), float(synth.CX)
    img = synth.render_room_depth(rows, cols, np.eye(3), np.zeros(3), fx, cx, 0.002, np.random.default_rng(7))
    out = {"frame": [rows, cols], "reps": a.reps, "warmup": a.warmup, "bytes_each_way": int(img.nbytes), "bilateral_us": {}}
    res = np.empty_like(img)
    with binding.Context(0) as ctx:
        out["filter_depth_image_us"] = timed(ctx, lambda: ctx.filter_depth_image(img), a.warmup, a.reps)
        for radius in (1, 3, 6):
            p = depth.bilateral_params(radius=radius, sigma_space=radius / 1.5)
            out["bilateral_us"][str(radius)] = timed(ctx, lambda: depth.bilateral_depth_image(ctx, img, p, out=res), a.warmup, a.reps)
        out["backproject_smoothed_us"] = timed(ctx, lambda: depth.backproject_smoothed(ctx, img, fx=fx, cx=cx), a.warmup, a.reps)
        out["backproject_us"] = timed(ctx, lambda: ctx.backproject(img, fx=fx, cx=cx), a.warmup, a.reps)
    line = json.dumps(out)
    print(line)
    prof = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
    os.makedirs(prof, exist_ok=True)
    with open(os.path.join(prof, "bilateral_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
