"""Cost of icpk_estimate_target_normals (include/icpk.h) next to two yardsticks taken in the same run:

  estimate      device span of one call (HIP events on the context's stream around it): with the target's grid index
                already there (the two K12 launches alone) and on a fresh target (the K1d index build included)
  grid sweep    the steady ICPK_NN_GRID sweep of the pair's source against the same target (same grid, seeded)
  image normals icpk_backproject_with_normals on the same frame, where the cloud has one

on config 2 (92k, r = 0.05), the dense 307k frame (r = 0.02) and config 5 (1M, r = 0.02).  Warm, median of --reps
(>= 5).  Every case runs in a child process of its own under a time limit; the first case that fails ends the run.
Prints one JSON line and writes it to --out.

    python tools/bench_normals.py [--reps 9] [--warmup 2] [--out profiles/normals_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from icp_slam_prototype_amd import binding, build, synth  # noqa: E402

CAM = (5.0, 5.0, 5.0)
CASES = {"config2_92k": 0.05, "dense_frame_307k": 0.02, "config5_1m": 0.02}
CASE_TIMEOUT_S = 240


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def run_case(name, reps, warmup):
    import torch

    radius = CASES[name]
    pair = {"config2_92k": synth.kinect_pair, "dense_frame_307k": lambda: synth.kinect_pair(valid=1.0, seed=6),
            "config5_1m": synth.dense_pair}[name]()
    tgt, src = pair["target"], pair["source"]
    rec = {"points": int(tgt.shape[1]), "radius": radius}
    with binding.Context(0) as ctx:
        stream = torch.cuda.ExternalStream(int(ctx.stream), device=torch.device("cuda", 0))

        def timed(prepare, fn):
            dev = []
            for k in range(warmup + reps):
                prepare()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if k >= warmup:
                    dev.append(1000.0 * e0.elapsed_time(e1))
            return round(median(dev), 1)

        ctx.set_target(tgt)
        ctx.set_source(src)
        rec["estimate_fresh_target_us"] = timed(lambda: ctx.set_target(tgt), lambda: ctx.estimate_target_normals(radius, 5, CAM))
        rec["estimate_index_present_us"] = timed(lambda: None, lambda: ctx.estimate_target_normals(radius, 5, CAM))
        st = ctx.get_normal_stats()
        rec["neighbours_per_point_mean"] = round(float(st["count"].mean()), 1)
        rec["neighbours_per_point_max"] = int(st["count"].max())
        rec["with_normal_share"] = round(st["n_valid"] / st["n"], 4)
        ctx.nn(binding.NN_GRID, fetch=False)   # (the first sweep: seeds for the steady ones)
        rec["grid_sweep_steady_us"] = timed(lambda: None, lambda: ctx.nn(binding.NN_GRID, fetch=False))
        if "depth_tgt" in pair:
            rec["backproject_with_normals_us"] = timed(
                lambda: None, lambda: ctx.backproject_with_normals(pair["depth_tgt"], binding.NORMALS_CROSS, offset=[5, 5, 5]))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_bench.json"))
    ap.add_argument("--case", choices=sorted(CASES), help="(internal) run one case in this process and print its record")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.case:
        print("RECORD " + json.dumps(run_case(a.case, a.reps, a.warmup)))
        return 0
    build.build()
    out = {"reps": a.reps, "warmup": a.warmup, "unit": "us of device span, median", "min_neighbors": 5}
    for name in CASES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(a.reps), "--warmup",
                                str(a.warmup)], capture_output=True, text=True, timeout=CASE_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {CASE_TIMEOUT_S} s; nothing further is started", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"{name}: exit status {r.returncode}; nothing further is started\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        out[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RECORD ")][-1][7:])
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
