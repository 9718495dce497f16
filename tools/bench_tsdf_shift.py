"""Timing of the moving volume (icpk_tsdf_shift / icpk_tsdf_extract_leaving, K23): the median over --reps calls after
--warmup calls, each call bracketed by HIP events on the context's stream (as tools/bench_tsdf_raycast.py).  Prints one
JSON line and writes it to profiles/tsdf_shift_bench.json.  No time is asserted anywhere.

Per volume (256^3 and 512^3 voxels over the same 5.12 m cube, voxel = 0.02 / 0.01 m, trunc = 4 voxels), one synthetic
640 x 480 frame of the room fused at the identity pose, then for s = (1, 0, 0), (4, 0, 0), (0, 0, 8):
  shift_us            icpk_tsdf_shift(s): the one kernel, no host wait (the shift is undone by nothing: the next call
                      shifts what the last one left, which costs the same -- every voxel is read and written once)
  floor_bytes         2 n 6: every voxel's tsdf and weight read once and written once (10 with colour)
  gbps / of_floor     floor_bytes over shift_us, and that over the 6.29 TB/s a float4 copy reaches on the card (8 TB/s on
                      the data sheet): the fraction of the byte floor the kernel reaches
  leaving_us          icpk_tsdf_extract_leaving(s): count, scan, the wait, scatter
  n_leaving           its list
and once: extract_us, icpk_tsdf_extract_surface next to it, and n_points.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from icp_slam_prototype_amd import binding, synth

COPY_GBPS = 6290.0
SHIFTS = [(1, 0, 0), (4, 0, 0), (0, 0, 8)]


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
    ap.add_argument("--dims", type=int, nargs="*", default=[256, 512])
    a = ap.parse_args()
    rows, cols = 480, 640
    fx, cx = float(synth.FX), float(synth.CX)
    P = np.eye(4)
    depth = synth.render_room_depth(rows, cols, P[:3, :3], P[:3, 3])
    out = {"frame": [rows, cols], "reps": a.reps, "warmup": a.warmup, "copy_gbps": COPY_GBPS, "volumes": []}
    with binding.Context(0) as ctx:
        for dim in a.dims:
            voxel = 5.12 / dim
            n = dim ** 3
            r = {"dims": [dim] * 3, "voxel": voxel, "floor_bytes": 2 * n * 6, "shifts": []}
            ctx.tsdf_create(dims=(dim,) * 3, voxel=voxel, origin=(-2.56, -2.56, 0.4), trunc=4 * voxel, max_weight=255)

            def refill():
                ctx.tsdf_reset()
                ctx.tsdf_integrate(depth, P, fx=fx, cx=cx)

            refill()
            r["n_points"], _ = ctx.tsdf_extract_surface(1)
            r["extract_us"] = timed(ctx, lambda: ctx.tsdf_extract_surface(1), a.warmup, a.reps)
            for s in SHIFTS:
                refill()
                e = {"s": list(s)}
                e["n_leaving"], _ = binding.tsdf_extract_leaving(ctx, s, 1)
                e["leaving_us"] = timed(ctx, lambda: binding.tsdf_extract_leaving(ctx, s, 1), a.warmup, a.reps)
                e["shift_us"] = timed(ctx, lambda: binding.tsdf_shift(ctx, s), a.warmup, a.reps)
                e["gbps"] = r["floor_bytes"] / e["shift_us"] / 1e3
                e["of_floor"] = e["gbps"] / COPY_GBPS
                r["shifts"].append(e)
            out["volumes"].append(r)
            ctx.tsdf_release()
    line = json.dumps(out)
    print(line)
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tsdf_shift_bench.json")
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
