"""Timing of the device certainty map (icpk_map_*, icpk_align_to_map): the median over --reps calls after --warmup
calls, each call bracketed by HIP events on the context's stream (an update ends with its one host wait, so the span
covers its 12 launches and the gaps between them).  Prints one JSON line.

  map_add_cloud_us      ADD_CLOUD, d = 180, over a 640 x 480 Kinect frame (~92k points; icp.cpp:62 / :270)
  map_add_unassoc_us    ADD_UNASSOCIATED, d = 25, over ~2k points (icp.cpp:271)
  map_tracker_frame_us  one steady-state MapTracker frame through the binding: key points back-projected and posed on
                        the host, uploaded, icpk_align_to_map (16 iterations max, threshold 1e-4), trace read back
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
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    out = {}
    rng = np.random.default_rng(0)
    with binding.Context(0) as ctx:
        ctx.map_reset()
        frame = synth.kinect_pair(rows=480, cols=640, valid=0.3, seed=2)["source"]
        ctx.set_source(frame)
        out["frame_points"] = int(frame.shape[1])
        out["map_add_cloud_us"] = timed(ctx, lambda: ctx.map_update(binding.MAP_ADD_CLOUD, 180, binding.MAP_FROM_SOURCE),
                                        a.warmup, a.reps)
        few = frame[:, rng.choice(frame.shape[1], 2000, replace=False)]
        ctx.set_source(few)
        out["map_add_unassoc_us"] = timed(ctx, lambda: ctx.map_update(binding.MAP_ADD_UNASSOCIATED, 25,
                                                                      binding.MAP_FROM_SOURCE), a.warmup, a.reps)
        # the live path: the map seeded by one frame's key points (icp.cpp:62), then the next frame against it
        ctx.map_reset()
        rows, cols = 480, 640
        d0 = synth.render_room_depth(rows, cols, np.eye(3), np.zeros(3), noise_sigma=0.001, rng=rng).astype(np.uint16)
        d1 = synth.render_room_depth(rows, cols, synth.rot_xyz_deg(0, 0.4, 0), np.array([0.01, 0, 0]), noise_sigma=0.001,
                                     rng=rng).astype(np.uint16)
        kp = np.stack([rng.uniform(4, cols - 5, 1500), rng.uniform(4, rows - 5, 1500)], 1).astype(np.float32)
        k0 = binding.backproject_keypoints(d0, kp)[0] + np.float32(5)
        ctx.map_update_points(binding.MAP_ADD_CLOUD, k0, 180)
        params = binding.default_params(max_nn_dist=0.1, max_iterations=16, threshold=1e-4, solve=0)
        n_key = ctx.map_size(binding.MAP_KEYPOINTS)

        def frame_step():
            ctx.map_reset()  # every timed frame meets the same map (not timed)
            ctx.map_update_points(binding.MAP_ADD_CLOUD, k0, 180)

        def tracker_frame():
            pts = binding.backproject_keypoints(d1, kp)[0] + np.float32(5)
            ctx.set_source(pts)
            ctx.align_to_map(params, delta=25)
            ctx.get_trace(16)

        stream = torch.cuda.ExternalStream(int(ctx.stream), device=torch.device("cuda", 0))
        us = []
        for r in range(a.warmup + a.reps):
            frame_step()
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            tracker_frame()
            e1.record(stream)
            e1.synchronize()
            if r >= a.warmup:
                us.append(1000.0 * e0.elapsed_time(e1))
        out["map_tracker_frame_us"] = float(np.median(us))
        out["map_keypoints"] = int(n_key)
        out["frame_keypoints"] = int(kp.shape[0])
    out["reps"] = a.reps
    print(json.dumps(out))


if __name__ == "__main__":
    main()
