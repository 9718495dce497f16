"""Timing of K32: oriented BRIEF descriptors (icpk_describe_keypoints), their Hamming matches (icpk_match_descriptors)
and the whole features.FrameRegistrar.register call.  The median over --reps calls after --warmup calls, each call
bracketed by HIP events on the context's stream, with the host wall time of the whole call beside it (as
tools/bench_fern.py).  Prints one JSON line and writes it to --out (profiles/brief_bench.json).  One run on one box: the
figures say what a frame pays there, nothing is asserted anywhere and there is no parent-commit counterpart.

The frames are the textured room of tests/brief_cases.py at 240 x 320 (about 3 000 key points at FAST threshold 20) and,
for the smaller and the larger list, the same frame at other thresholds; the key-point counts are in the output.
  describe_us[n]      icpk_describe_keypoints on a resident detection of n key points: one copy of the list, one launch
  match_us[n]         icpk_match_descriptors of n x n descriptors, mutual, H <= 48, with the count read back: two match
                      launches, the finish launch, one copy, one wait
  match_oneway_us[n]  the same without ICPK_BRIEF_MUTUAL: one match launch
  register_wall_us    FrameRegistrar.register of two frames, host wall time: two detections, two describes, two clouds, the
                      match, 4096 RANSAC hypotheses scored by K15, and (register_refined_wall_us) the dense ICP refinement
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from icp_slam_prototype_amd import binding
from icp_slam_prototype_amd import features as F
from icp_slam_prototype_amd.features import FrameRegistrar


def timed(ctx, fn, warmup, reps):
    """(median microseconds between the events, median microseconds of host wall time)"""
    stream = torch.cuda.ExternalStream(int(ctx.stream), device=torch.device("cuda", 0))
    us, wall = [], []
    for k in range(warmup + reps):
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
    ap.add_argument("--thresholds", type=int, nargs="*", default=[40, 20, 12])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "brief_bench.json"))
    a = ap.parse_args()
    import brief_cases as bc

    (bgr_a, depth_a), (bgr_b, depth_b) = bc.frame(None), bc.frame("yaw24")
    out = {"frame": [bc.ROWS, bc.COLS], "reps": a.reps, "warmup": a.warmup, "note": "one run on one box", "keypoints": {},
           "describe_us": {}, "describe_wall_us": {}, "match_us": {}, "match_wall_us": {}, "match_oneway_us": {},
           "match_oneway_wall_us": {}, "kept": {}}
    with binding.Context(0) as ctx:
        lib, h = ctx._lib, ctx._h
        n_out = C.c_int32(0)
        for t in a.thresholds:
            counts = []
            for which, bgr in enumerate((bgr_a, bgr_b)):
                ctx.detect_fast(bgr, threshold=t, capacity=0)
                counts.append(ctx.detected_count)
                F.describe_keypoints(ctx, which)
            key = str(counts[1])
            out["keypoints"][str(t)] = counts
            # (the second frame's detection is resident: describe it again and again)
            out["describe_us"][key], out["describe_wall_us"][key] = timed(ctx, lambda: lib.icpk_describe_keypoints(h, 1, 0), a.warmup, a.reps)
            for name, mutual in (("match", True), ("match_oneway", False)):
                p = binding.brief_match_params(max_hamming=48, mutual=mutual)
                us, wall = timed(ctx, lambda: lib.icpk_match_descriptors(h, C.byref(p), C.byref(n_out)), a.warmup, a.reps)
                out[name + "_us"][key], out[name + "_wall_us"][key] = us, wall
                if mutual:
                    out["kept"][key] = n_out.value
        for name, refine in (("register_wall_us", False), ("register_refined_wall_us", True)):
            reg = FrameRegistrar(ctx, fx=bc.FX, cx=bc.CX, fast_threshold=bc.FAST_THRESHOLD, max_dist=0.05, refine=refine)
            wall = []
            for k in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                r = reg.register(bgr_a, depth_a, bgr_b, depth_b)
                if k >= a.warmup:
                    wall.append(1e6 * (time.perf_counter() - t0))
            out[name] = float(np.median(wall))
            out["register_inliers"] = int(r["inliers"])
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
