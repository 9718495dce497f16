"""Cost of voxel-grid downsampling (include/icpk.h, icpk_voxel_downsample), all in one process so that
the figures share a machine and a run:

  downsample   device span of one call (HIP events on the context's stream around it: the table clear, the five
               launches, the read-back of the two counts, the copies into the cloud) and the host's wall clock around
               it -- 92k Kinect cloud, 1M dense cloud, and 200 000 points in ONE voxel; leaf 0.05, both modes
  (a) index    for comparison, the existing per-cloud indexing on the same clouds: icpk_set_target_device + the first
               ICPK_NN_GRID sweep of a 64-point source (the grid build; the scan of 64 queries is negligible)
  (b) loop     one align of 20 fixed iterations (Kabsch, device loop) on the full pair against downsample-both + the
               same align on the result; wall clock from resident clouds to the returned transform

Warm, median of --reps (>= 20).  Prints one JSON line and writes it to --out.

    python tools/bench_voxel.py [--reps 25] [--warmup 3] [--out profiles/voxel_downsample.json]
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_voxel.py --only-calls --out /dev/null
        (kernel times, in a run of its own: only the downsample calls, nothing else on the device)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from icp_slam_prototype_amd import binding, build, synth  # noqa: E402

LEAF = 0.05
ITERS = 20
MODES = (("first", binding.VOXEL_FIRST), ("centroid", binding.VOXEL_CENTROID))


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_downsample.json"))
    ap.add_argument("--only-calls", action="store_true", help="the downsample calls alone (for a kernel trace)")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    build.build()
    rng = np.random.default_rng(1)
    one = np.minimum(rng.uniform(1.0, 1.25, (3, 200_000)).astype(np.float32), np.nextafter(np.float32(1.25), np.float32(0)))
    kin, den = synth.kinect_pair(), synth.dense_pair()
    out = {"leaf": LEAF, "reps": a.reps, "warmup": a.warmup, "unit": "us, median", "iterations_of_b": ITERS}
    with binding.Context(0) as ctx:
        stream = torch.cuda.ExternalStream(int(ctx.stream), device=torch.device("cuda", 0))

        def timed(prepare, fn):
            """(device span, host wall clock) of fn(), both medians in us; prepare() runs untimed before every call"""
            dev, wall = [], []
            for k in range(a.warmup + a.reps):
                prepare()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                t0 = time.perf_counter()
                fn()
                e1.record(stream)
                e1.synchronize()
                t1 = time.perf_counter()
                if k >= a.warmup:
                    dev.append(1000.0 * e0.elapsed_time(e1))
                    wall.append(1e6 * (t1 - t0))
            return round(median(dev), 1), round(median(wall), 1)

        # ---- the call itself
        clouds = (("kinect_92k", kin["target"], 0.05), ("dense_1m", den["target"], 0.05), ("one_voxel_200k", one, 0.25))
        for name, pts, leaf in clouds:
            rec = {"points": int(pts.shape[1]), "leaf": leaf}
            for mname, mode in MODES:
                n_out = [0]

                def call():
                    n_out[0] = ctx.voxel_downsample(1, leaf, mode)[0]

                d, w = timed(lambda: ctx.set_target(pts), call)
                rec[mname] = {"device_span_us": d, "wall_us": w, "n_out": n_out[0]}
            out[name] = rec
        if a.only_calls:
            print(json.dumps(out))
            return
        # ---- (a) the existing per-cloud indexing
        tiny = np.ascontiguousarray(kin["source"][:, :64])
        for name, pts in (("kinect_92k", kin["target"]), ("dense_1m", den["target"])):
            dev_t = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
            n = pts.shape[1]

            def index():
                ctx.set_target_device(dev_t[0].data_ptr(), dev_t[1].data_ptr(), dev_t[2].data_ptr(), n)
                ctx.nn(binding.NN_GRID, fetch=False)

            d, w = timed(lambda: ctx.set_source(tiny), index)
            out[name]["a_set_target_device_plus_first_grid_sweep"] = {"device_span_us": d, "wall_us": w}
        # ---- (b) the loop on the full pair against downsample-both + the loop on the result
        params = binding.default_params(solve=binding.SOLVE_KABSCH, max_iterations=ITERS, fixed_iterations=1)
        for name, pair in (("kinect_92k", kin), ("dense_1m", den)):
            def load():
                ctx.set_target(pair["target"])
                ctx.set_source(pair["source"])

            res = {}

            def full():
                res["full"] = ctx.align(params)

            def thinned():
                ctx.voxel_downsample(1, LEAF, binding.VOXEL_CENTROID)
                ctx.voxel_downsample(0, LEAF, binding.VOXEL_CENTROID)
                res["thin"] = ctx.align(params)

            df, wf = timed(load, full)
            dt, wt = timed(load, thinned)
            assert res["full"][2] == 0 and res["thin"][2] == 0
            out[name]["b_align20_full"] = {"device_span_us": df, "wall_us": wf, "final_pairs": res["full"][1].final_pairs}
            out[name]["b_downsample_both_plus_align20"] = {"device_span_us": dt, "wall_us": wt,
                                                           "final_pairs": res["thin"][1].final_pairs,
                                                           "T_difference_frobenius": float(np.linalg.norm(
                                                               res["full"][0].astype(np.float64) - res["thin"][0].astype(np.float64)))}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
