"""Timing of K9, the mapped nearest-neighbour lookup, at 640 x 480: the median over --reps calls after --warmup calls,
each bracketed by HIP events on the context's stream.  The map is seeded as the live path seeds it from a rendered room
(the key points of a textured colour frame through ADD_CLOUD, the frame's cloud as the point list) and then thickened by
one dense fold (ADD_ASSOCIATED over the next frame's cloud, twice).  Prints one JSON line.

  sweep_sub40_us      one ICPK_NN_MAP sweep (icpk_nn, nothing copied out) for the 1-in-40 subsample of the next frame
  sweep_full_us       the same for the full cloud of that frame
  dense_frame_us      icpk_align_to_map_dense end to end for the subsample (16 iterations max, threshold 1e-4, fold
                      with d = 25 included; the map re-seeded, untimed, before every call)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import fast_model as fm
from icp_slam_prototype_amd import binding, synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    rows, cols = 480, 640
    rng = np.random.default_rng(0)
    R0, c0 = np.eye(3), np.zeros(3)
    R1, c1 = synth.rot_xyz_deg(0, 0.4, 0), np.array([0.01, 0.0, 0.005])
    d0 = synth.render_room_depth(rows, cols, R0, c0, noise_sigma=0.001, rng=rng).astype(np.uint16)
    d1 = synth.render_room_depth(rows, cols, R1, c1, noise_sigma=0.001, rng=rng).astype(np.uint16)
    col0 = np.ascontiguousarray(synth.render_room_color(rows, cols, R0, c0, noise_sigma=2.0, rng=rng))
    kp, _ = fm.detect(col0, 60, True, fm.TYPE_7_12)
    k0 = binding.backproject_keypoints(d0, kp)[0] + np.float32(5)
    I3 = np.eye(3, dtype=np.float32)
    P5 = np.full(3, 5, np.float32)
    params = binding.default_params(max_nn_dist=0.75, max_iterations=16, threshold=1e-4, solve=0)
    out = {"rows": rows, "cols": cols}
    with binding.Context(0) as ctx:
        stream = torch.cuda.ExternalStream(int(ctx.stream), device=torch.device("cuda", 0))

        def span(fn):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            return 1000.0 * e0.elapsed_time(e1)

        def seed():
            ctx.map_reset()
            ctx.map_update_points(binding.MAP_ADD_CLOUD, k0, 180)
            ctx.backproject(d0, which=1)
            ctx.transform_target(I3, P5)
            ctx.map_set_points(binding.MAP_FROM_TARGET)
            ctx.backproject(d1, which=1)
            ctx.transform_target(I3, P5)
            ctx.map_update(binding.MAP_ADD_ASSOCIATED, 255, binding.MAP_FROM_TARGET)
            ctx.map_update(binding.MAP_ADD_ASSOCIATED, 255, binding.MAP_FROM_TARGET)

        def source(factor):
            ctx.set_subsample(factor, 3)
            ctx.backproject(d1, which=0)
            ctx.transform_source(I3, P5)
            ctx.commit_source()
            return ctx.source_size

        seed()
        out["map_keypoints"] = ctx.map_size(binding.MAP_KEYPOINTS)
        out["map_points"] = ctx.map_size(binding.MAP_POINTS)
        for name, factor in (("sub40", 40), ("full", 1)):
            out[f"queries_{name}"] = source(factor)
            ctx.map_lookup_to_target()
            ts = [span(lambda: ctx.nn(binding.NN_MAP, fetch=False)) for _ in range(a.warmup + a.reps)]
            out[f"sweep_{name}_us"] = float(np.median(ts[a.warmup:]))
        source(40)
        ts = []
        for _ in range(a.warmup + a.reps):
            seed()
            ts.append(span(lambda: ctx.align_to_map_dense(params, delta=25)))
        out["dense_frame_us"] = float(np.median(ts[a.warmup:]))
        T, st, rc = ctx.align_to_map_dense(params, delta=0)
        out["dense_iterations"] = int(st.iterations)
        out["dense_final_pairs"] = int(st.final_pairs)
    out["reps"] = a.reps
    print(json.dumps(out))


if __name__ == "__main__":
    main()
