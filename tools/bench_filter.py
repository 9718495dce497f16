"""Cost of icpk_remove_outliers (include/icpk.h) next to two yardsticks taken in the same run:

  statistical   device span of one ICPK_FILTER_STATS_ONLY call on the target (HIP events on the context's stream around
                it) with the target's grid index already there: the k-NN kernel, the two sums, the threshold and the
                compaction; k = 8, 16, 50
  radius        the same for ICPK_FILTER_RADIUS at the case's radius
  estimate      K12's icpk_estimate_target_normals at the same radius, index present
  grid sweep    the steady ICPK_NN_GRID sweep of the pair's source against the same target (same grid, seeded)

on config 2 (92k, r = 0.05), the dense 307k frame (r = 0.02) and config 5 (1M, r = 0.02).  Warm, median of --reps
(>= 5).  Every case runs in a child process of its own under a time limit; the first case that fails ends the run.
Prints one JSON line and writes it to --out.

    python tools/bench_filter.py [--reps 9] [--warmup 2] [--out profiles/filter_bench.json]
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
        ctx.estimate_target_normals(radius, 5, CAM)  # (builds the index)
        for k in (8, 16, 50):
            rec[f"statistical_k{k}_us"] = timed(lambda: None, lambda: ctx.remove_outliers(1, k=k, std_ratio=2.0, stats_only=True))
            rec[f"statistical_k{k}_kept_share"] = round(ctx.outlier_stats()["n_out"] / tgt.shape[1], 4)
        rec["radius_us"] = timed(lambda: None, lambda: ctx.remove_outliers(1, kind=binding.FILTER_RADIUS, radius=radius,
                                                                          min_neighbors=5, stats_only=True))
        rec["neighbours_per_point_mean"] = round(float(ctx.outlier_stats()["value"].mean()), 1)
        rec["estimate_index_present_us"] = timed(lambda: None, lambda: ctx.estimate_target_normals(radius, 5, CAM))
        ctx.nn(binding.NN_GRID, fetch=False)   # (the first sweep: seeds for the steady ones)
        rec["grid_sweep_steady_us"] = timed(lambda: None, lambda: ctx.nn(binding.NN_GRID, fetch=False))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_bench.json"))
    ap.add_argument("--case", choices=sorted(CASES), help="(internal) run one case in this process and print its record")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.case:
        print("RECORD " + json.dumps(run_case(a.case, a.reps, a.warmup)))
        return 0
    build.build()
    out = {"reps": a.reps, "warmup": a.warmup, "unit": "us of device span, median"}
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
