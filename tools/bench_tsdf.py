"""Timing of the TSDF volume (icpk_tsdf_*, K19): the median over --reps calls after --warmup calls, each call bracketed
by HIP events on the context's stream (as tools/bench_map.py).  Prints one JSON line and writes it to
profiles/tsdf_bench.json.

Per volume (256^3 and 512^3 voxels over the same 5.12 m cube, so voxel = 0.02 / 0.01 m, trunc = 4 voxels), one synthetic
640 x 480 frame of the room (synth.render_room_depth):
  integrate_us            icpk_tsdf_integrate with a host depth image: the upload, both kernels and the wait for n_updated
  integrate_resident_us   ... with the frame icpk_backproject_pair left on the device and no count asked: the two kernels
  n_updated               voxels written per frame
  bytes_touched           12 bytes per written voxel: tsdf and weight read and written (the 614 KB image is gathered
                          and sits in L2; a voxel that fails a test touches nothing of the volume)
  resident_gbps           bytes_touched / integrate_resident_us
  sweep_gbps              the same time against the bytes a plain sweep of both planes would move (6 bytes per voxel):
                          how the kernel compares with streaming the volume once
  extract_us              icpk_tsdf_extract_surface after three frames: count, scan, the wait, scatter
  n_points / n_no_normal  what it listed / dropped
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from icp_slam_prototype_amd import binding, synth


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


def pose(rot, shift):
    P = np.eye(4)
    P[:3, :3] = synth.rot_xyz_deg(*rot)
    P[:3, 3] = shift
    return P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dims", type=int, nargs="*", default=[256, 512])
    a = ap.parse_args()
    rows, cols = 480, 640
    fx, cx = float(synth.FX), float(synth.CX)
    motions = [((0, 0, 0), (0, 0, 0)), ((0, 2, 0), (0.03, 0, 0)), ((1, -2, 0), (-0.02, 0.02, 0.01))]
    poses = [pose(*m) for m in motions]
    frames = [synth.render_room_depth(rows, cols, P[:3, :3], P[:3, 3]) for P in poses]
    out = {"frame": [rows, cols], "reps": a.reps, "warmup": a.warmup, "volumes": []}
    with binding.Context(0) as ctx:
        for dim in a.dims:
            voxel = 5.12 / dim
            r = {"dims": [dim] * 3, "voxel": voxel, "trunc": 4 * voxel, "origin": [-2.56, -2.56, 0.4]}
            ctx.tsdf_create(dims=(dim,) * 3, voxel=voxel, origin=r["origin"], trunc=4 * voxel, max_weight=255)
            r["n_updated"] = ctx.tsdf_integrate(frames[0], poses[0], fx=fx, cx=cx)
            r["integrate_us"] = timed(ctx, lambda: ctx.tsdf_integrate(frames[0], poses[0], fx=fx, cx=cx), a.warmup, a.reps)
            ctx.backproject_pair(frames[0], frames[1], fx=fx, cx=cx)  # (frames[0] is the resident frame now)
            r["integrate_resident_us"] = timed(
                ctx, lambda: ctx.tsdf_integrate(None, poses[0], fx=fx, cx=cx, shape=(rows, cols), count=False), a.warmup, a.reps)
            n = dim ** 3
            r["bytes_touched"] = 12 * r["n_updated"]
            r["resident_gbps"] = r["bytes_touched"] / r["integrate_resident_us"] / 1e3
            r["sweep_gbps"] = 6 * n / r["integrate_resident_us"] / 1e3
            ctx.tsdf_reset()
            for d, P in zip(frames, poses):
                ctx.tsdf_integrate(d, P, fx=fx, cx=cx)
            r["n_points"], r["n_no_normal"] = ctx.tsdf_extract_surface(1)
            r["extract_us"] = timed(ctx, lambda: ctx.tsdf_extract_surface(1), a.warmup, a.reps)
            ctx.tsdf_release()
            out["volumes"].append(r)
    line = json.dumps(out)
    print(line)
    prof = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
    os.makedirs(prof, exist_ok=True)
    with open(os.path.join(prof, "tsdf_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
