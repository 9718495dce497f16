"""Timing of fern keyframe relocalisation (icpk_fern_process, K27): the median over --reps calls after --warmup calls,
each call bracketed by HIP events on the context's stream, with the host wall time of the whole call beside it (as
tools/bench_pyramid.py).  Prints one JSON line and writes it to profiles/fern_bench.json.  One run on one box: the
figures say what a frame pays there, nothing is asserted anywhere.

The level is level 2 (30 x 40) of the 120 x 160 room of tests/tsdf_cases.py with sensor noise; the database holds n random
codes (icpk_fern_add_code), so every keyframe is scanned in full.
  process_us[F][n]        icpk_fern_process without a pose: encode, search, merge, one copy, one wait (n = 0: encode alone)
  encode_us[F]            icpk_fern_encode: the encode launch, the copy of the code and V, the wait -- what a host search
                          would still pay before it could start; process_us - encode_us is what the device search adds
  harvest_us[F]           icpk_fern_process with a pose on an empty database: the call that appends
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
    ap.add_argument("--sizes", type=int, nargs="*", default=[0, 64, 4096, 65536])
    a = ap.parse_args()
    import tsdf_cases as tc

    img = synth.render_room_depth(*tc.ROOM_SHAPE, np.eye(3), np.zeros(3), tc.ROOM_FX, tc.ROOM_CX, 0.002, np.random.default_rng(27))
    out = {"frame": list(tc.ROOM_SHAPE), "level": 2, "reps": a.reps, "warmup": a.warmup, "k": 3, "note": "one run on one box",
           "process_us": {}, "process_wall_us": {}, "encode_us": {}, "encode_wall_us": {}, "harvest_us": {}, "harvest_wall_us": {}}
    eye = np.eye(4)
    with binding.Context(0) as ctx:
        depth.build_pyramid(ctx, img, depth.pyramid_params(levels=3))
        for F in (256, 1024):
            out["process_us"][str(F)], out["process_wall_us"][str(F)] = {}, {}
            for n in a.sizes:
                binding.fern_create(ctx, 30, 40, n_ferns=F, capacity=max(n, 1))
                codes = np.random.default_rng(n + F).integers(0, 2 ** 32, (n, F // 8), dtype=np.uint32)
                for code in codes:
                    binding.fern_add_code(ctx, code, eye)
                us, wall = timed(ctx, lambda: binding.fern_process(ctx, None, 3), a.warmup, a.reps)
                out["process_us"][str(F)][str(n)], out["process_wall_us"][str(F)][str(n)] = us, wall
            out["encode_us"][str(F)], out["encode_wall_us"][str(F)] = timed(ctx, lambda: binding.fern_encode(ctx), a.warmup, a.reps)
            binding.fern_create(ctx, 30, 40, n_ferns=F, capacity=4)
            out["harvest_us"][str(F)], out["harvest_wall_us"][str(F)] = timed(ctx, lambda: binding.fern_process(ctx, eye, 3), a.warmup,
                                                                              a.reps, before=lambda: binding.fern_reset(ctx))
        binding.fern_destroy(ctx)
    line = json.dumps(out)
    print(line)
    prof = os.path.join(ROOT, "profiles")
    os.makedirs(prof, exist_ok=True)
    with open(os.path.join(prof, "fern_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
