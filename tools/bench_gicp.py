"""Cost of the plane-to-plane flavour (include/icpk.h, ICPK_SOLVE_PLANE_TO_PLANE) on the config-3
full-size pair of tests/test_gpu_full_iterations.py (424 x 512, every pixel valid), next to its yardsticks taken in the
same run:

  (a) kernels   rocprofv3 --kernel-trace --stats over a child that alternates icpk_reduce_p2l and
                icpk_reduce_plane_to_plane on the same associations: the kernel time of gicp_reduce_kernel beside
                p2l_reduce_kernel<28>.  A run of its own (no counters, no other tracing).
  (b) loop      iterations/s of a 20-iteration fixed alignment, plane-to-plane beside point-to-plane, same pair, same
                estimated target normals, ICPK_NN_GRID, device loop; host clock around calls that end in the result
                being read, alternating the two flavours, median of --reps.
  (c) normals   device span (HIP events on the context's stream) of icpk_estimate_source_normals beside
                icpk_estimate_target_normals on the same cloud and radius; the target's index is present, the source's
                is rebuilt by every call (it owns no persistent one).

Every part runs in a child process of its own under a time limit; the first that fails ends the run.  Prints one JSON
line and writes it to --out.

    python tools/bench_gicp.py [--reps 9] [--warmup 2] [--out profiles/gicp_bench.json]
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


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from icp_slam_prototype_amd import binding, build, synth  # noqa: E402

RADIUS, MIN_NB, MAX_D, ITERS = 0.03, 5, 0.3, 20
PART_TIMEOUT_S = 240


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def pair():
    fx, cx = float(synth.K2_FX), float(synth.K2_CX)
    return synth.kinect_pair(rows=424, cols=512, valid=1.0, seed=2, fx=fx, cx=cx)


def prepared(ctx):
    p = pair()
    ctx.set_target(p["target"])
    ctx.set_source(p["source"])
    ctx.estimate_target_normals(RADIUS, MIN_NB)
    ctx.estimate_source_normals(RADIUS, MIN_NB)
    return p


def part_hooks(reps, warmup):
    """the child rocprofv3 traces: both reductions over the same associations, alternating"""
    with binding.Context(0) as ctx:
        prepared(ctx)
        ctx.nn(binding.NN_GRID, fetch=False)
        for _ in range(warmup + reps):
            ctx.reduce_p2l(MAX_D)
            ctx.reduce_plane_to_plane(MAX_D)
    return {}


def part_kernels(reps, warmup):
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "-o", "p", "--", sys.executable,
               os.path.abspath(__file__), "--part", "hooks", "--reps", str(reps), "--warmup", str(warmup)]
        subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=PART_TIMEOUT_S - 20)
        files = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        rec = {}
        for r in csv.DictReader(open(files[0])):
            for key, name in (("gicp_reduce_kernel", "gicp_reduce"), ("p2l_reduce_kernel<28>", "p2l_reduce_28")):
                if key in r["Name"]:
                    rec[name + "_calls"] = int(r["Calls"])
                    rec[name + "_avg_us"] = round(float(r["AverageNs"]) / 1e3, 2)
                    rec[name + "_min_us"] = round(float(r["MinNs"]) / 1e3, 2)
    return rec


def part_loop(reps, warmup):
    rec = {}
    with binding.Context(0) as ctx:
        p = prepared(ctx)
        rec["points"] = int(p["source"].shape[1])
        kw = dict(max_iterations=ITERS, fixed_iterations=1, max_nn_dist=MAX_D, nn_mode=binding.NN_GRID)
        wall = {binding.SOLVE_POINT_TO_PLANE: [], binding.SOLVE_PLANE_TO_PLANE: []}
        for k in range(warmup + reps):
            for solve in wall:  # alternating
                t0 = time.perf_counter()
                T, st, rc = ctx.align(solve=solve, **kw)  # (returns when T and the statistics are final)
                dt = time.perf_counter() - t0
                assert rc == 0 and st.iterations == ITERS
                if k >= warmup:
                    wall[solve].append(dt)
        for solve, name in ((binding.SOLVE_POINT_TO_PLANE, "point_to_plane"), (binding.SOLVE_PLANE_TO_PLANE, "plane_to_plane")):
            m = median(wall[solve])
            rec[name + "_ms"] = round(1e3 * m, 3)
            rec[name + "_iterations_per_s"] = round(ITERS / m, 1)
            rec[name + "_spread_ms"] = [round(1e3 * min(wall[solve]), 3), round(1e3 * max(wall[solve]), 3)]
    return rec


def part_normals(reps, warmup):
    import torch

    rec = {"radius": RADIUS}
    with binding.Context(0) as ctx:
        p = pair()
        cloud = p["target"]
        ctx.set_target(cloud)
        ctx.set_source(cloud)
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

        ctx.estimate_target_normals(RADIUS, MIN_NB)  # (builds the target's index)
        rec["estimate_target_index_present_us"] = timed(lambda: ctx.estimate_target_normals(RADIUS, MIN_NB))
        rec["estimate_source_with_its_index_us"] = timed(lambda: ctx.estimate_source_normals(RADIUS, MIN_NB))
        rec["with_a_normal_share"] = round(float((ctx.get_source_normals() != 0).any(0).mean()), 4)
    return rec


PARTS = {"hooks": part_hooks, "kernels": part_kernels, "loop": part_loop, "normals": part_normals}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gicp_bench.json"))
    ap.add_argument("--part", choices=sorted(PARTS), help="(internal) run one part in this process and print its record")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.part:
        print("RECORD " + json.dumps(PARTS[a.part](a.reps, a.warmup)))
        return 0
    build.build()
    out = {"reps": a.reps, "warmup": a.warmup, "pair": "config 3 full size (424 x 512, every pixel valid)"}
    for name in ("kernels", "loop", "normals"):
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
