"""Timing of the mesh extraction of the TSDF volume (icpk_tsdf_extract_mesh, K21): the median over --reps calls after
--warmup calls, each call bracketed by HIP events on the context's stream (the set-up and protocol of
tools/bench_tsdf_raycast.py).  Prints one JSON line and writes it to profiles/tsdf_mesh_bench.json.

Per volume (256^3 and 512^3 voxels over the same 5.12 m cube, so voxel = 0.02 / 0.01 m, trunc = 4 voxels), one synthetic
640 x 480 frame of the room fused at the identity pose:
  extract_mesh_us         icpk_tsdf_extract_mesh: count, two scans, the wait for the counts, the two scatters
  extract_surface_us      icpk_tsdf_extract_surface in the same run: K19's walk over the same voxels
  ratio                   extract_mesh_us / extract_surface_us
  sweep_bytes             6 n: the tsdf and the weight plane read once
  n_vertices / n_triangles / n_no_normal, n_points   what either call listed
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
    out = {"frame": [rows, cols], "reps": a.reps, "warmup": a.warmup, "volumes": []}
    with binding.Context(0) as ctx:
        for dim in a.dims:
            voxel = 5.12 / dim
            r = {"dims": [dim] * 3, "voxel": voxel, "trunc": 4 * voxel, "origin": [-2.56, -2.56, 0.4], "sweep_bytes": 6 * dim ** 3}
            ctx.tsdf_create(dims=(dim,) * 3, voxel=voxel, origin=r["origin"], trunc=4 * voxel, max_weight=255)
            ctx.tsdf_integrate(depth, P, fx=fx, cx=cx)
            r["n_vertices"], r["n_triangles"], r["n_no_normal"] = ctx.tsdf_extract_mesh(1)
            r["n_points"], _ = ctx.tsdf_extract_surface(1)
            r["extract_mesh_us"] = timed(ctx, lambda: ctx.tsdf_extract_mesh(1), a.warmup, a.reps)
            r["extract_surface_us"] = timed(ctx, lambda: ctx.tsdf_extract_surface(1), a.warmup, a.reps)
            r["ratio"] = r["extract_mesh_us"] / r["extract_surface_us"]
            ctx.tsdf_release()
            out["volumes"].append(r)
    line = json.dumps(out)
    print(line)
    prof = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
    os.makedirs(prof, exist_ok=True)
    with open(os.path.join(prof, "tsdf_mesh_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
