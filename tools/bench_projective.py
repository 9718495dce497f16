"""Timing of projective frame-to-model alignment (K25) next to the cloud-to-cloud tracker it stands beside: medians over
--reps calls after --warmup calls, each call bracketed by HIP events on the context's stream with the host wall time of
the whole call next to them (a track call is mostly launches and host waits).  The compared paths ALTERNATE inside one
process: round k runs every path once before round k + 1 begins.  Prints one JSON line and writes it to
profiles/projective_bench.json.  One run on one box: the figures say what a frame pays there, nothing is asserted.

track_*: one ModelTracker.track call of the fourth room frame from the third pose, against the three frames fused at their
true poses, the model put back before every call (untimed).
  plain_19            max_iterations = 19, max_nn_dist = 0.1
  pyramid_10_5_4      pyramid = (10, 5, 4), the same gate
  projective_19       projective = True, max_iterations = 19, max_dist = 0.5
  projective_10_5_4   projective = True, pyramid = (10, 5, 4), max_dist = 0.5
at 120 x 160 against the 64^3 volume of tests/tsdf_cases.py, and at 480 x 640 against a 256^3 volume of 2 cm voxels.
level_*: at 120 x 160, per level l of a (10, 5, 4) pyramid with the ray cast already made: align_projective alone, next to
raycast_to_target + backproject_level + transform + commit + align, which it replaces.
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

TRACKERS = (("plain_19", dict(max_iterations=19, max_nn_dist=0.1)),
            ("pyramid_10_5_4", dict(pyramid=(10, 5, 4), max_nn_dist=0.1)),
            ("projective_19", dict(projective=dict(max_dist=0.5), max_iterations=19)),
            ("projective_10_5_4", dict(projective=dict(max_dist=0.5), pyramid=(10, 5, 4))))


def alternate(ctx, paths, warmup, reps):
    """paths: [(key, before, fn)].  Round by round, every path once.  Returns {key: (median event us, median wall us)}"""
    stream = torch.cuda.ExternalStream(int(ctx.stream), device=torch.device("cuda", 0))
    us, wall = {k: [] for k, _, _ in paths}, {k: [] for k, _, _ in paths}
    for r in range(warmup + reps):
        for key, before, fn in paths:
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
            if r >= warmup:
                us[key].append(1000.0 * e0.elapsed_time(e1))
                wall[key].append(1e6 * (t1 - t0))
    return {k: (float(np.median(us[k])), float(np.median(wall[k]))) for k, _, _ in paths}


def track_paths(ctx, geom, fx, cx, frames, d4, P3):
    vol = TsdfVolume(ctx, **geom, fx=fx, cx=cx)
    for d, P in frames:
        vol.integrate(d, P)
    model = vol.planes()[:2]
    paths = []
    for key, extra in TRACKERS:
        state = {}

        def before(state=state, extra=extra):
            vol.set_planes(*model)
            state["t"] = ModelTracker(vol, pose=P3, step=0.125 if geom["dims"][0] == 64 else None, **extra)
            state["t"].frames = 3

        paths.append((key, before, lambda state=state: state["t"].track(d4)))
    return vol, model, paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-vga", action="store_true", help="leave out the 480 x 640 / 256^3 part")
    a = ap.parse_args()
    import tsdf_cases as tc

    out = {"reps": a.reps, "warmup": a.warmup, "note": "one run on one box; medians; the paths alternate round by round"}
    c = tc.case("room")
    geom = {k: c["volume"][k] for k in ("dims", "voxel", "origin", "trunc")}
    d4, _ = tc.room_frame(*tc.ROOM_FOURTH)
    P3 = c["frames"][2][1]
    with binding.Context(0) as ctx:
        vol, model, paths = track_paths(ctx, geom, c["fx"], c["cx"], [(d, P) for d, P, _ in c["frames"]], d4, P3)
        res = alternate(ctx, paths, a.warmup, a.reps)
        out["track_120x160"] = {k: {"events_us": v[0], "wall_us": v[1]} for k, v in res.items()}
        # per level: the projective loop alone next to what it replaces, the ray cast already made
        vol.set_planes(*model)
        counts = (10, 5, 4)
        shapes = depth.build_pyramid(ctx, d4, depth.pyramid_params(levels=3))
        out["level_120x160"] = {}
        for l in (2, 1, 0):
            scale = float(2 ** l)
            ray = binding.tsdf_raycast_params(shape=shapes[l], fx=c["fx"] / scale, cx=c["cx"] / scale, z_near=0.25, z_far=6.0,
                                              step=0.125, min_weight=1)
            jp = binding.default_projective_params(level=l, fx=c["fx"], cx=c["cx"], max_iterations=counts[l], max_dist=0.5)
            ap_ = binding.default_params(solve=binding.SOLVE_POINT_TO_PLANE, max_iterations=counts[l], max_nn_dist=0.1 * scale)

            def cloud_path():
                ctx.tsdf_raycast_to_target()
                depth.backproject_level(ctx, l, which=0, fx=c["fx"], cx=c["cx"])
                ctx.transform_source(P3[:3, :3], P3[:3, 3])
                ctx.commit_source()
                ctx.align(ap_)

            cast = lambda: ctx.tsdf_raycast(P3, ray)
            res = alternate(ctx, [("align_projective", cast, lambda: binding.align_projective(ctx, P3, jp)), ("to_target_backproject_align", cast, cloud_path)],
                            a.warmup, a.reps)
            out["level_120x160"][str(l)] = {"shape": list(shapes[l]), "iterations": counts[l],
                                            **{k: {"events_us": v[0], "wall_us": v[1]} for k, v in res.items()}}
    if not a.skip_vga:
        rows, cols = 480, 640
        fx, cx = float(synth.FX), float(synth.CX)
        render = lambda m: (synth.render_room_depth(rows, cols, tc.pose(*m)[:3, :3], tc.pose(*m)[:3, 3], fx, cx), tc.pose(*m))
        frames = [render(m) for m in tc.ROOM_MOTIONS]
        big = dict(dims=(256, 256, 256), voxel=0.02, origin=(-2.56, -2.56, 0.0), trunc=0.08)
        with binding.Context(0) as ctx:
            _, _, paths = track_paths(ctx, big, fx, cx, frames, render(tc.ROOM_FOURTH)[0], frames[2][1])
            res = alternate(ctx, paths, a.warmup, a.reps)
            out["track_480x640_256"] = {k: {"events_us": v[0], "wall_us": v[1]} for k, v in res.items()}
    line = json.dumps(out)
    print(line)
    prof = os.path.join(ROOT, "profiles")
    os.makedirs(prof, exist_ok=True)
    with open(os.path.join(prof, "projective_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
