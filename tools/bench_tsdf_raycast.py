"""Timing of the ray cast of the TSDF volume (icpk_tsdf_raycast*, K20): the median over --reps calls after --warmup
calls, each call bracketed by HIP events on the context's stream (as tools/bench_tsdf.py).  Prints one JSON line and
writes it to profiles/tsdf_raycast_bench.json.

Per volume (256^3 and 512^3 voxels over the same 5.12 m cube, so voxel = 0.02 / 0.01 m, trunc = 4 voxels), one synthetic
640 x 480 frame of the room fused at the identity pose and seen again from there, 0.25 .. 6 m in steps of trunc / 2:
  samples                 N, the samples a ray may take
  raycast_us              icpk_tsdf_raycast without a count: the kernel and the two slot sums, no host wait
  raycast_counted_us      ... with both counts: the same and the wait for them
  raycast_to_target_us    icpk_tsdf_raycast + icpk_tsdf_raycast_to_target: count, scan, the wait, scatter, the copies
  n_hits / n_no_normal    what the ray cast listed / dropped: n_hits is the target's size
  extract_to_target_us    the route to a model target without a ray cast: icpk_tsdf_extract_surface (a walk over all
                          voxels, one wait) + icpk_tsdf_surface_to_target
  n_points                the surface list's size: that target's size
  align_raycast_us / align_surface_us   one point-to-plane icpk_align (20 iterations at most, 0.2 m) of the frame's own
                          cloud, moved by 2 cm, against either target
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
    src = synth.backproject(depth, None, fx, cx).astype(np.float32) + np.float32([[0.02], [0.0], [0.0]])
    akw = dict(solve=binding.SOLVE_POINT_TO_PLANE, max_iterations=20, max_nn_dist=0.2)
    out = {"frame": [rows, cols], "reps": a.reps, "warmup": a.warmup, "volumes": []}
    with binding.Context(0) as ctx:
        for dim in a.dims:
            voxel = 5.12 / dim
            r = {"dims": [dim] * 3, "voxel": voxel, "trunc": 4 * voxel, "origin": [-2.56, -2.56, 0.4]}
            ctx.tsdf_create(dims=(dim,) * 3, voxel=voxel, origin=r["origin"], trunc=4 * voxel, max_weight=255)
            ctx.tsdf_integrate(depth, P, fx=fx, cx=cx)
            ray = binding.tsdf_raycast_params(shape=(rows, cols), fx=fx, cx=cx, z_near=0.25, z_far=6.0, step=2 * voxel)
            r["samples"] = int(np.floor((6.0 - 0.25) / float(np.float32(2 * voxel)))) + 1
            r["n_hits"], r["n_no_normal"] = ctx.tsdf_raycast(P, ray)
            r["raycast_us"] = timed(ctx, lambda: ctx.tsdf_raycast(P, ray, count=False), a.warmup, a.reps)
            r["raycast_counted_us"] = timed(ctx, lambda: ctx.tsdf_raycast(P, ray), a.warmup, a.reps)

            def to_target():
                ctx.tsdf_raycast(P, ray, count=False)
                ctx.tsdf_raycast_to_target()

            r["raycast_to_target_us"] = timed(ctx, to_target, a.warmup, a.reps)
            ctx.set_source(src)
            r["align_raycast_us"] = timed(ctx, lambda: ctx.align(**akw), a.warmup, a.reps)

            def extract_to_target():
                ctx.tsdf_extract_surface(1)
                ctx.tsdf_surface_to_target()

            r["n_points"], _ = ctx.tsdf_extract_surface(1)
            r["extract_to_target_us"] = timed(ctx, extract_to_target, a.warmup, a.reps)
            ctx.set_source(src)
            r["align_surface_us"] = timed(ctx, lambda: ctx.align(**akw), a.warmup, a.reps)
            ctx.tsdf_release()
            out["volumes"].append(r)
    line = json.dumps(out)
    print(line)
    prof = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
    os.makedirs(prof, exist_ok=True)
    with open(os.path.join(prof, "tsdf_raycast_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
