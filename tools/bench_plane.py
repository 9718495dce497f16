"""Cost of icpk_segment_planes (include/icpk.h) next to its yardstick taken in the same run:

  plane     device span of one ICPK_PLANE_LABELS_ONLY call on the target (HIP events on the context's stream around it):
            every round's launches AND the host wait between two rounds, which the span contains because the next round is
            enqueued only after the host has read the count block
  radius    the same for K13's ICPK_FILTER_RADIUS | ICPK_FILTER_STATS_ONLY call on the same cloud (radius 0.05, 5
            neighbours), whose code this feature does not touch

on config 2's target (92k), the dense 307k frame and config 5's 1M target, at 256 and 4 096 hypotheses per round
(t 0.01, max_planes 4, min_inliers 5 % of the cloud, seed 0).  Warm, median of --reps (>= 5).  Next to each span the floor
the code implies, computed from the rounds' own counts: sum over the rounds of m H 10 float64 operations (3 subtractions,
4 multiplications, 2 additions and the compare's square are what plane_score_kernel does per test; none is fused) over
FP64_OPS_PER_S, and the bytes of E read once per chunk of 64 hypotheses, sum of 16 m ceil(H / 64), over HBM_BYTES_PER_S.
Every case runs in a child process of its own under a time limit; the first case that fails ends the run.  Prints one
JSON line and writes it to --out.

    python tools/bench_plane.py [--reps 9] [--warmup 2] [--out profiles/plane_bench.json]

--case NAME --hyp H --once runs three labels-only calls of a case and nothing else, for a kernel trace of the launches:
the first allocates the buffers, the other two are warm.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from icp_slam_prototype_amd import binding, build, planes, synth  # noqa: E402

CASES = ("config2_92k", "dense_frame_307k", "config5_1m")
HYPOTHESES = (256, 4096)
CASE_TIMEOUT_S = 240
# the MI355X's published vector FP64 peak is 78.6 TFLOP/s with every operation a fused multiply-add (2 per lane and
# clock); the rule forbids fusing, so an unfused multiply or add retires at half of that
FP64_OPS_PER_S = 78.6e12 / 2
HBM_BYTES_PER_S = 8.0e12
PL_HCHUNK = 64  # kernels_plane.hip


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def target_of(name):
    return {"config2_92k": synth.kinect_pair, "dense_frame_307k": lambda: synth.kinect_pair(valid=1.0, seed=6),
            "config5_1m": synth.dense_pair}[name]()["target"]


def settings(n, hyp):
    return dict(distance_threshold=0.01, n_hypotheses=hyp, max_planes=4, min_inliers=max(3, n // 20), seed=0)


def run_once(name, hyp):
    tgt = target_of(name)
    with binding.Context(0) as ctx:
        ctx.set_target(tgt)
        for _ in range(3):  # (the first allocates the buffers)
            counts = planes.segment(ctx, 1, labels_only=True, **settings(tgt.shape[1], hyp))
    return {"planes": counts[0], "unassigned": counts[1]}


def run_case(name, hyp, reps, warmup):
    import torch

    tgt = target_of(name)
    n = int(tgt.shape[1])
    kw = settings(n, hyp)
    rec = {"points": n, "n_hypotheses": hyp, "min_inliers": kw["min_inliers"]}
    with binding.Context(0) as ctx:
        stream = torch.cuda.ExternalStream(int(ctx.stream), device=torch.device("cuda", 0))

        def timed(fn):
            dev = []
            for k in range(warmup + reps):
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
        ctx.remove_outliers(1, kind=binding.FILTER_RADIUS, radius=0.05, min_neighbors=5, stats_only=True)  # (builds the index)
        rec["radius_us"] = timed(lambda: ctx.remove_outliers(1, kind=binding.FILTER_RADIUS, radius=0.05, min_neighbors=5,
                                                             stats_only=True))
        rec["plane_us"] = timed(lambda: planes.segment(ctx, 1, labels_only=True, **kw))
        r = planes.planes(ctx)
        rec["planes"], rec["final_counts"] = r["n_planes"], r["info"][:, 5].tolist()
        # the rounds that ran: one per plane, and the one that ended the call if it was started (m >= 3 and >= min_inliers)
        m, ms = int(np.isfinite(tgt).all(0).sum()), []
        for f in rec["final_counts"]:
            ms.append(m)
            m -= f
        if len(ms) < kw["max_planes"] and m >= max(3, kw["min_inliers"]):
            ms.append(m)
        rec["rounds"], rec["open_points_per_round"] = len(ms), ms
        ops = sum(10.0 * v * hyp for v in ms)
        byts = sum(16.0 * v * -(-hyp // PL_HCHUNK) for v in ms)
        rec["count_float64_ops"], rec["count_bytes_read"] = ops, byts
        rec["floor_us_fp64"] = round(1e6 * ops / FP64_OPS_PER_S, 2)
        rec["floor_us_bytes"] = round(1e6 * byts / HBM_BYTES_PER_S, 2)
        rec["plane_over_radius"] = round(rec["plane_us"] / rec["radius_us"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_bench.json"))
    ap.add_argument("--case", choices=CASES, help="(internal) run one case in this process and print its record")
    ap.add_argument("--hyp", type=int, default=256, help="with --case: hypotheses per round")
    ap.add_argument("--once", action="store_true", help="with --case: three labels-only calls (one cold, two warm) and nothing else")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.case:
        print("RECORD " + json.dumps(run_once(a.case, a.hyp) if a.once else run_case(a.case, a.hyp, a.reps, a.warmup)))
        return 0
    build.build()
    out = {"reps": a.reps, "warmup": a.warmup, "unit": "us of device span (the rounds' host waits included), median",
           "fp64_ops_per_s_assumed": FP64_OPS_PER_S, "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S}
    for name in CASES:
        for hyp in HYPOTHESES:
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--hyp", str(hyp), "--reps", str(a.reps),
                                    "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=CASE_TIMEOUT_S)
            except subprocess.TimeoutExpired:
                print(f"{name} H={hyp}: no result within {CASE_TIMEOUT_S} s; nothing further is started", file=sys.stderr)
                return 1
            if r.returncode != 0:
                print(f"{name} H={hyp}: exit status {r.returncode}; nothing further is started\n{r.stderr[-2000:]}", file=sys.stderr)
                return 1
            out[f"{name}_h{hyp}"] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RECORD ")][-1][7:])
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
