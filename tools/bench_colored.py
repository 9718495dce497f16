"""Cost of colored ICP (include/icpk.h, icpk_set_colored) on the config-3 full-size pair of
tests/test_gpu_full_iterations.py (424 x 512, every pixel valid) with a synthetic intensity per point, next to its
yardsticks taken in the same run:

  (a) kernels    rocprofv3 --kernel-trace --stats over a child that alternates icpk_reduce_p2l and icpk_reduce_colored
                 on the same associations: the kernel time of colored_reduce_kernel beside p2l_reduce_kernel<28>.  A run
                 of its own (no counters, no other tracing).
  (b) loop       iterations/s of a 20-iteration fixed alignment, colored beside plain point-to-plane, same pair, same
                 estimated target normals, ICPK_NN_GRID, device loop; host clock around calls that end in the result
                 being read, alternating the two, median of --reps.
  (c) gradients  device span (HIP events on the context's stream) of icpk_estimate_target_color_gradients beside
                 icpk_estimate_target_normals on the same target and radius, the target's index present.

Every part runs in a child process of its own under a time limit; the first that fails ends the run.  Prints one JSON
line and writes it to --out.

    python tools/bench_colored.py [--reps 9] [--warmup 2] [--out profiles/colored_bench.json]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from icp_slam_prototype_amd import binding, build, synth  # noqa: E402

RADIUS, MIN_NB, MAX_D, ITERS, LAMBDA = 0.03, 5, 0.3, 20, 0.968
PART_TIMEOUT_S = 240


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def intensity(pts):
    """a smooth texture over the room's coordinates, in [0.05, 0.95]"""
    x, y, z = (pts[k].astype(np.float64) for k in range(3))
    return (0.5 + 0.25 * np.sin(2 * np.pi * (x + 0.5 * z) / 0.2) + 0.2 * np.cos(2 * np.pi * y / 0.15)).astype(np.float32)


def pair():
    fx, cx = float(synth.K2_FX), float(synth.K2_CX)
    return synth.kinect_pair(rows=424, cols=512, valid=1.0, seed=2, fx=fx, cx=cx)


def prepared(ctx):
    p = pair()
    R, t = np.asarray(p["R_true"], np.float64), np.asarray(p["t_true"], np.float64)
    ctx.set_target(p["target"])
    ctx.set_source(p["source"])
    ctx.estimate_target_normals(RADIUS, MIN_NB)
    ctx.set_target_colors(intensity(p["target"]))
    # the source's texture is the target's seen from the moved camera (to first order: the pair's true motion)
    moved = (R @ (p["source"].astype(np.float64) - 5.0) + t[:, None] + 5.0).astype(np.float32)
    ctx.set_source_colors(intensity(moved))
    ctx.estimate_target_color_gradients(RADIUS, MIN_NB)
    return p


def part_hooks(reps, warmup):
    """the child rocprofv3 traces: both reductions over the same associations, alternating"""
    with binding.Context(0) as ctx:
        prepared(ctx)
        ctx.set_colored(False, LAMBDA)
        ctx.nn(binding.NN_GRID, fetch=False)
        for _ in range(warmup + reps):
            ctx.reduce_p2l(MAX_D)
            ctx.reduce_colored(MAX_D)
    return {}


def part_kernels(reps, warmup):
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "-o", "p", "--", sys.executable,
               os.path.abspath(__file__), "--part", "hooks", "--reps", str(reps), "--warmup", str(warmup)]
        subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=PART_TIMEOUT_S - 20)
        files = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no *kernel_stats.csv under its output directory")
        rec = {}
        for r in csv.DictReader(open(files[0])):
            for key, name in (("colored_reduce_kernel", "colored_reduce"), ("p2l_reduce_kernel<28>", "p2l_reduce_28")):
                if key in r["Name"]:
                    rec[name + "_calls"] = int(r["Calls"])
                    rec[name + "_avg_us"] = round(float(r["AverageNs"]) / 1e3, 2)
                    rec[name + "_min_us"] = round(float(r["MinNs"]) / 1e3, 2)
        for name in ("colored_reduce", "p2l_reduce_28"):
            if name + "_calls" not in rec:
                raise RuntimeError(f"{files[0]} has no row for the {name} kernel")
    return rec


def part_loop(reps, warmup):
    rec = {}
    with binding.Context(0) as ctx:
        p = prepared(ctx)
        rec["points"] = int(p["source"].shape[1])
        kw = dict(solve=binding.SOLVE_POINT_TO_PLANE, max_iterations=ITERS, fixed_iterations=1, max_nn_dist=MAX_D,
                  nn_mode=binding.NN_GRID)
        wall = {False: [], True: []}
        for k in range(warmup + reps):
            for colored in wall:  # alternating
                ctx.set_colored(colored, LAMBDA)
                t0 = time.perf_counter()
                T, st, rc = ctx.align(**kw)  # (returns when T and the statistics are final)
                dt = time.perf_counter() - t0
                assert rc == 0 and st.iterations == ITERS
                if k >= warmup:
                    wall[colored].append(dt)
        for colored, name in ((False, "point_to_plane"), (True, "colored")):
            m = median(wall[colored])
            rec[name + "_ms"] = round(1e3 * m, 3)
            rec[name + "_iterations_per_s"] = round(ITERS / m, 1)
            rec[name + "_spread_ms"] = [round(1e3 * min(wall[colored]), 3), round(1e3 * max(wall[colored]), 3)]
    return rec


def part_gradients(reps, warmup):
    import torch

    rec = {"radius": RADIUS}
    with binding.Context(0) as ctx:
        prepared(ctx)
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

        rec["estimate_color_gradients_us"] = timed(lambda: ctx.estimate_target_color_gradients(RADIUS, MIN_NB))
        rec["with_a_gradient_share"] = round(float((ctx.get_target_color_gradients() != 0).any(0).mean()), 4)
        # (last: it replaces the normals; the index stays)
        rec["estimate_target_normals_us"] = timed(lambda: ctx.estimate_target_normals(RADIUS, MIN_NB))
    return rec


PARTS = {"hooks": part_hooks, "kernels": part_kernels, "loop": part_loop, "gradients": part_gradients}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colored_bench.json"))
    ap.add_argument("--part", choices=sorted(PARTS), help="(internal) run one part in this process and print its record")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.part:
        print("RECORD " + json.dumps(PARTS[a.part](a.reps, a.warmup)))
        return 0
    build.build()
    out = {"reps": a.reps, "warmup": a.warmup, "pair": "config 3 full size (424 x 512, every pixel valid), synthetic texture"}
    for name in ("kernels", "loop", "gradients"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", name, "--reps", str(a.reps), "--warmup",
                                str(a.warmup)], capture_output=True, text=True, timeout=PART_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {PART_TIMEOUT_S} s; nothing further is started", file=sys.stderr)
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
