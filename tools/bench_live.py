"""Timing of the live path with device FAST (K8) at 640 x 480: the median over --reps calls after --warmup calls, each
bracketed by HIP events on the context's stream (every call ends with its host wait, so the span covers its launches
and the gaps between them).  Prints one JSON line.

  fast_detect_us           icpk_detect_fast on a BGR frame (upload, 3 launches, count back; no key points copied out)
  detected_to_cloud_us     icpk_detected_to_cloud: the detected list back-projected, posed, made the source
  live_frame_fast_us       one live frame end to end with device FAST: detect, detected_to_cloud, icpk_align_to_map
                           (16 iterations max, threshold 1e-4), trace read back
  live_frame_hostkp_us     the same frame through the existing path, the key points detected by the model beforehand
                           and handed in: host back-projection and pose, upload, icpk_align_to_map, trace read back
The two live variants alternate call by call; the map is re-seeded (not timed) before every timed frame.
"""
import argparse
import ctypes as C
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
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    rows, cols = 480, 640
    rng = np.random.default_rng(0)
    R0, c0 = np.eye(3), np.zeros(3)
    R1, c1 = synth.rot_xyz_deg(0, 0.4, 0), np.array([0.01, 0.0, 0.005])
    d0 = synth.render_room_depth(rows, cols, R0, c0, noise_sigma=0.001, rng=rng).astype(np.uint16)
    d1 = synth.render_room_depth(rows, cols, R1, c1, noise_sigma=0.001, rng=rng).astype(np.uint16)
    col1 = np.ascontiguousarray(synth.render_room_color(rows, cols, R1, c1, noise_sigma=2.0, rng=rng))
    kp, _ = fm.detect(col1, 60, True, fm.TYPE_7_12)
    I3 = np.eye(3, dtype=np.float32)
    P5 = np.full(3, 5, np.float32)
    k0 = binding.backproject_keypoints(d0, kp)[0] + np.float32(5)
    params = binding.default_params(max_nn_dist=0.1, max_iterations=16, threshold=1e-4, solve=0)
    out = {"rows": rows, "cols": cols, "keypoints": int(len(kp))}
    u8, ip, fp = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_float)
    with binding.Context(0) as ctx:
        lib, h = ctx._lib, ctx._h
        stream = torch.cuda.ExternalStream(int(ctx.stream), device=torch.device("cuda", 0))
        img_p = col1.ctypes.data_as(u8)
        d1_p = d1.ctypes.data_as(C.POINTER(C.c_uint16))
        Rf, tf = I3.reshape(9).copy(), P5.copy()
        n = np.zeros(1, np.int32)

        def detect():
            assert lib.icpk_detect_fast(h, img_p, rows, cols, 3, 60, 1, binding.FAST_TYPE_7_12, 0, None, None,
                                        n.ctypes.data_as(ip)) == 0

        def to_cloud():
            assert lib.icpk_detected_to_cloud(h, d1_p, rows, cols, 468.60, 318.27, Rf.ctypes.data_as(fp),
                                              tf.ctypes.data_as(fp), 0, n.ctypes.data_as(ip)) == 0

        def live_fast():
            detect()
            to_cloud()
            ctx.align_to_map(params, delta=25)
            ctx.get_trace(16)

        def live_host():
            ctx.set_source(binding.backproject_keypoints(d1, kp)[0] + np.float32(5))  # (pose: identity, (5, 5, 5))
            ctx.align_to_map(params, delta=25)
            ctx.get_trace(16)

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

        times = {"fast_detect_us": [], "detected_to_cloud_us": [], "live_frame_fast_us": [], "live_frame_hostkp_us": []}
        for r in range(a.warmup + a.reps):
            t_det = span(detect)
            t_cloud = span(to_cloud)
            seed()
            t_fast = span(live_fast)
            seed()
            t_host = span(live_host)
            if r >= a.warmup:
                for k, v in zip(times, (t_det, t_cloud, t_fast, t_host)):
                    times[k].append(v)
        detect()
        out["detected"] = int(n[0])
        to_cloud()
        out["cloud_points"] = int(n[0])
        for k, v in times.items():
            out[k] = float(np.median(v))
    out["reps"] = a.reps
    print(json.dumps(out))


if __name__ == "__main__":
    main()
