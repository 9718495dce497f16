#!/usr/bin/env python
"""Diagnostic: what one pass over the TSDF volume for several frames (K30, icpk_tsdf_apply) costs next to one pass per
frame (the unchanged icpk_tsdf_integrate).

For 64^3 and 256^3 volumes over the same four metres of the room, with and without colour, at 120 x 160 and 480 x 640:
n calls of icpk_tsdf_integrate against one icpk_tsdf_apply with the same n +1 ops, n = 1, 2, 8, 16 -- the same frames
uploaded, the same poses; the two give the same bytes, which is asserted on a fresh volume before anything is timed --
and TsdfVolume.refuse of 8 frames (8 removals and 8 integrations in one pass).  Medians of `reps` calls after `warmup`,
HIP events on the context's stream and wall time around the same calls.  Nothing is asserted about time; one run on one
box says what the order of magnitude is, not more.

    python tools/bench_tsdf_refuse.py [--reps 10] [--warmup 2] [--out profiles/tsdf_refuse_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # (before the library: both bring a HIP runtime, and torch's must be the first initialised)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tsdf_cases as tc  # noqa: E402
from icp_slam_prototype_amd import binding  # noqa: E402
from icp_slam_prototype_amd.tsdf import TsdfVolume  # noqa: E402

NS = (1, 2, 8, 16)
VOLUMES = {64: dict(dims=(64, 64, 64), voxel=0.0625, origin=(-2.3, -1.9, 0.4), trunc=0.25),
           256: dict(dims=(256, 256, 256), voxel=0.015625, origin=(-2.3, -1.9, 0.4), trunc=0.0625)}


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def frames_at(shape, color):
    """sixteen frames of the room at `shape`, the field of view kept: four rendered views, each at four poses a few
    millimetres apart (the rule does not care whether a pose is the true one): (fx, cx, depths, poses, intensities)"""
    fx, cx = tc.ROOM_FX * shape[1] / tc.ROOM_SHAPE[1], tc.ROOM_CX * shape[1] / tc.ROOM_SHAPE[1]
    motions = list(tc.ROOM_MOTIONS) + [tc.ROOM_FOURTH]
    views = [tc.room_frame(*m, shape=shape, fx=fx, cx=cx) for m in motions]
    inten = [tc.room_intensity(*m, shape=shape, fx=fx, cx=cx) for m in motions] if color else None
    depths, poses, images = [], [], []
    for k in range(16):
        d, P = views[k % 4]
        depths.append(d)
        poses.append(P @ tc.pose((0.1 * (k // 4), 0.0, 0.0), (0.002 * (k // 4), 0.0, 0.0)))
        if color:
            images.append(inten[k % 4])
    return fx, cx, depths, poses, images if color else None


def timed(ctx, fn, reps, warmup):
    stream = torch.cuda.ExternalStream(int(ctx.stream), device=torch.device("cuda", 0))
    dev, wall = [], []
    for k in range(warmup + reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        dt = time.perf_counter() - t0
        if k >= warmup:
            dev.append(e0.elapsed_time(e1))
            wall.append(1000.0 * dt)
    return dict(device_ms=round(median(dev), 4), wall_ms=round(median(wall), 4))


def measure(side, color, shape, reps, warmup):
    fx, cx, depths, poses, inten = frames_at(shape, color)
    rec = {"volume": side, "color": color, "shape": list(shape), "n": {}}
    with binding.Context(0) as ctx:
        vol = TsdfVolume(ctx, color=color, fx=fx, cx=cx, **VOLUMES[side])

        def one_by_one(n):
            for k in range(n):
                ctx.tsdf_integrate(depths[k], poses[k], None if inten is None else inten[k], fx=fx, cx=cx, count=False)

        def batched(n):
            vol.apply(depths[:n], [(+1, k, poses[k]) for k in range(n)], None if inten is None else inten[:n])

        for n in NS:
            vol.reset()
            one_by_one(n)
            want = vol.planes(intensity=color)
            vol.reset()
            batched(n)
            got = vol.planes(intensity=color)
            assert all(a is None or a.tobytes() == b.tobytes() for a, b in zip(want, got)), (side, color, shape, n)
            a = timed(ctx, lambda: one_by_one(n), reps, warmup)
            b = timed(ctx, lambda: batched(n), reps, warmup)
            rec["n"][str(n)] = {"integrate_calls": a, "one_apply": b,
                                "apply_over_integrate_device": round(b["device_ms"] / a["device_ms"], 3),
                                "apply_over_integrate_wall": round(b["wall_ms"] / a["wall_ms"], 3)}
        vol.reset()
        one_by_one(8)
        moved = [P @ tc.pose((0.0, 0.5, 0.0), (0.01, 0.0, 0.0)) for P in poses[:8]]
        state = {"old": poses[:8], "new": moved}

        def refuse():
            vol.refuse(depths[:8], state["old"], state["new"], None if inten is None else inten[:8])
            state["old"], state["new"] = state["new"], state["old"]  # (there and back: the volume stays what it holds)

        rec["refuse_8_frames"] = timed(ctx, refuse, reps, warmup)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_refuse_bench.json"))
    a = ap.parse_args()
    runs = [measure(side, color, shape, a.reps, a.warmup)
            for side in (64, 256) for color in (False, True) for shape in ((120, 160), (480, 640))]
    out = {"command": f"python tools/bench_tsdf_refuse.py --reps {a.reps} --warmup {a.warmup}",
           "note": "medians; one run on one MI355X: an order of magnitude, not a comparison to rely on; every pair of "
                   "timed paths gave the same bytes on a fresh volume",
           "runs": runs}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
