"""Timing of the photometric term in projective frame-to-model alignment (K26) next to the geometric path it stands
beside (K25), in the manner of tools/bench_projective.py: medians over --reps calls after --warmup calls, each call
bracketed by HIP events on the context's stream with the host wall time of the whole call next to them.  The compared
paths ALTERNATE inside one process: round k runs every path once before round k + 1 begins.  Prints one JSON line and
writes it to profiles/projective_color_bench.json.  One run on one box: nothing is asserted.

level_*: per level l of a (10, 5, 4) pyramid of the 120 x 160 colour room, the ray cast already made:
  align_projective / align_projective_colored   the two loops, counts[l] iterations
  raycast / raycast_color_gradients             the gradient launch beside the ray cast it follows
pyramid_120x160: depth.build_pyramid (3 levels) beside binding.set_pyramid_intensity on the resident pyramid.
track_*: one ModelTracker.track call of the fourth room frame from the third pose, against the three frames fused at
their true poses into a colour volume, the model put back before every call (untimed), with and without
projective_color, at 120 x 160 / 64^3 and at 480 x 640 / 256^3 (2 cm voxels).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from bench_projective import alternate
from icp_slam_prototype_amd import binding, depth, synth
from icp_slam_prototype_amd.tsdf import ModelTracker, TsdfVolume

TRACKERS = (("projective_19", dict(max_iterations=19)), ("projective_colored_19", dict(max_iterations=19, projective_color=True)),
            ("projective_10_5_4", dict(pyramid=(10, 5, 4))), ("projective_colored_10_5_4", dict(pyramid=(10, 5, 4), projective_color=True)))


def intensity_of(bgr):
    return (bgr.astype(np.float64).sum(-1) / 765.0).astype(np.float32)


def track_paths(ctx, geom, fx, cx, frames, d4, i4, P3):
    vol = TsdfVolume(ctx, **geom, color=True, fx=fx, cx=cx)
    for d, P, inten in frames:
        vol.integrate(d, P, inten)
    model = vol.planes(intensity=True)
    paths = []
    for key, extra in TRACKERS:
        state = {}

        def before(state=state, extra=extra):
            vol.set_planes(*model)
            state["t"] = ModelTracker(vol, pose=P3, step=0.125 if geom["dims"][0] == 64 else None, projective=dict(max_dist=0.5), **extra)
            state["t"].frames = 3

        paths.append((key, before, lambda state=state: state["t"].track(d4, i4)))
    return vol, model, paths


def fields(res):
    return {k: {"events_us": v[0], "wall_us": v[1]} for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-vga", action="store_true", help="leave out the 480 x 640 / 256^3 part")
    a = ap.parse_args()
    import tsdf_cases as tc

    out = {"reps": a.reps, "warmup": a.warmup, "note": "one run on one box; medians; the paths alternate round by round"}
    c = tc.case("room_color")
    geom = {k: c["volume"][k] for k in ("dims", "voxel", "origin", "trunc")}
    voxel = geom["voxel"]
    d4, _ = tc.room_frame(*tc.ROOM_FOURTH)
    i4 = tc.room_intensity(*tc.ROOM_FOURTH)
    P3 = c["frames"][2][1]
    with binding.Context(0) as ctx:
        vol, model, paths = track_paths(ctx, geom, c["fx"], c["cx"], c["frames"], d4, i4, P3)
        out["track_120x160"] = fields(alternate(ctx, paths, a.warmup, a.reps))
        vol.set_planes(*model)
        pp = depth.pyramid_params(levels=3)
        out["pyramid_120x160"] = fields(alternate(
            ctx, [("build_pyramid", None, lambda: depth.build_pyramid(ctx, d4, pp)),
                  ("set_pyramid_intensity", None, lambda: binding.set_pyramid_intensity(ctx, i4))], a.warmup, a.reps))
        counts = (10, 5, 4)
        shapes = depth.build_pyramid(ctx, d4, pp, intensity=i4)
        out["level_120x160"] = {}
        for l in (2, 1, 0):
            scale = float(2 ** l)
            ray = binding.tsdf_raycast_params(shape=shapes[l], fx=c["fx"] / scale, cx=c["cx"] / scale, z_near=0.25, z_far=6.0,
                                              step=0.125, min_weight=1)
            jp = binding.default_projective_params(level=l, fx=c["fx"], cx=c["cx"], max_iterations=counts[l], max_dist=0.5)
            cast = lambda: ctx.tsdf_raycast(P3, ray, count=False)
            grads = lambda: binding.raycast_color_gradients(ctx, 2 * voxel * scale, 4)

            def cast_and_grads():
                cast()
                grads()

            res = alternate(ctx, [("raycast", None, cast), ("raycast_color_gradients", cast, grads),
                                  ("align_projective", cast_and_grads, lambda: binding.align_projective(ctx, P3, jp)),
                                  ("align_projective_colored", cast_and_grads, lambda: binding.align_projective_colored(ctx, P3, jp))],
                            a.warmup, a.reps)
            out["level_120x160"][str(l)] = {"shape": list(shapes[l]), "iterations": counts[l], **fields(res)}
    if not a.skip_vga:
        rows, cols = 480, 640
        fx, cx = float(synth.FX), float(synth.CX)

        def render(m):
            P = tc.pose(*m)
            return (synth.render_room_depth(rows, cols, P[:3, :3], P[:3, 3], fx, cx), P,
                    intensity_of(synth.render_room_color(rows, cols, P[:3, :3], P[:3, 3], fx, cx)))

        frames = [render(m) for m in tc.ROOM_MOTIONS]
        big = dict(dims=(256, 256, 256), voxel=0.02, origin=(-2.56, -2.56, 0.0), trunc=0.08)
        f4 = render(tc.ROOM_FOURTH)
        with binding.Context(0) as ctx:
            _, _, paths = track_paths(ctx, big, fx, cx, frames, f4[0], f4[2], frames[2][1])
            out["track_480x640_256"] = fields(alternate(ctx, paths, a.warmup, a.reps))
    line = json.dumps(out)
    print(line)
    prof = os.path.join(ROOT, "profiles")
    os.makedirs(prof, exist_ok=True)
    with open(os.path.join(prof, "projective_color_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
