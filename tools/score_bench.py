"""Cost of icpk_score_poses (include/icpk.h) next to the calls a user had before it, in the same run and
on the same build:

  score     one Context.score_poses call for n poses: upload of the poses, the search over poses x points, the sums,
            one host wait
  baseline  per pose reset_source, transform_source, nn(NN_GRID, fetch=False), reduce -- four calls and two host
            waits per candidate, the working source and the associations overwritten

on the 640 x 480, 30 %-valid synthetic pair of the headline, max_dist in {0.1, 0.75}, n in {1, 16, 64, 256} poses: small
perturbations of the true motion, every fourth pose far off.  Host clock around calls that end in a host wait; warm;
the two paths alternate; median, minimum and maximum of --reps (>= 5).  The rows run in a child process under a time
limit.  --count: with a diagnostic build (-DICPK_SCORE_COUNT) the candidates the search evaluated per (pose, point).
Prints one JSON line and writes it to --out.

    python tools/score_bench.py [--reps 7] [--warmup 2] [--count] [--out profiles/score_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from icp_slam_prototype_amd import build, synth  # noqa: E402

MAX_DISTS = (0.1, 0.75)
N_POSES = (1, 16, 64, 256)
TIMEOUT_S = 540
COUNT_LIB = os.path.join(build.HERE, "lib_variants", "libicpk_score_count.so")


def poses(pair, n, seed=3):
    """(n, 4, 4) float32: the true motion perturbed by ~0.3 degrees and ~5 mm; every fourth pose by ~20 degrees and ~1 m"""
    rng = np.random.default_rng(seed)
    c = np.full(3, 5.0)
    out = []
    for k in range(n):
        far = k % 4 == 3
        dR = synth.rot_xyz_deg(*rng.normal(0, 20.0 if far else 0.3, 3))
        R = dR @ pair["R_true"]
        t = pair["t_true"] + c - R @ c + rng.normal(0, 1.0 if far else 0.005, 3)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, t
        out.append(T)
    return np.asarray(out, np.float32)


def stats(v):
    v = sorted(v)
    return {"median_ms": round(1e3 * v[len(v) // 2], 3), "min_ms": round(1e3 * v[0], 3), "max_ms": round(1e3 * v[-1], 3)}


def run_rows(reps, warmup, count):
    from icp_slam_prototype_amd import binding

    pair = synth.kinect_pair()
    src, tgt = pair["source"], pair["target"]
    rows = []
    with binding.Context(0) as new, binding.Context(0) as old:
        for c in (new, old):
            c.set_target(tgt)
            c.set_source(src)
        for max_dist in MAX_DISTS:
            for n in N_POSES:
                T = poses(pair, n)

                def score():
                    return new.score_poses(T, max_dist)

                def baseline():
                    cnt = []
                    for k in range(n):
                        old.reset_source()
                        old.transform_source(T[k][:3, :3], T[k][:3, 3])
                        old.nn(binding.NN_GRID, fetch=False)
                        cnt.append(old.reduce(max_dist)[1])
                    return cnt

                ts, tb = [], []
                for k in range(warmup + reps):
                    t0 = time.perf_counter()
                    out = score()
                    t1 = time.perf_counter()
                    cnt = baseline()
                    t2 = time.perf_counter()
                    if k >= warmup:
                        ts.append(t1 - t0)
                        tb.append(t2 - t1)
                assert list(out["inliers"]) == cnt, "the two paths count different inliers"
                row = {"max_dist": max_dist, "n_poses": n, "source_points": int(src.shape[1]),
                       "target_points": int(tgt.shape[1]), "score": stats(ts), "baseline": stats(tb),
                       "mean_fitness_near": round(float(np.mean([f for k, f in enumerate(out["fitness"]) if k % 4 != 3])), 4)}
                row["speedup_median"] = round(row["baseline"]["median_ms"] / row["score"]["median_ms"], 2)
                if count:
                    w = (C.c_ulonglong * 2)()
                    new._lib.icpk_debug_read_score_count(w)  # (clears the counters)
                    score()
                    new._lib.icpk_debug_read_score_count(w)
                    row["candidates_per_point"] = round(w[0] / (n * src.shape[1]), 1)
                    row["rounds_per_point"] = round(w[1] / (n * src.shape[1]), 2)
                    near = [k for k in range(n) if k % 4 != 3]
                    new.score_poses(T[near], max_dist)
                    new._lib.icpk_debug_read_score_count(w)
                    row["candidates_per_point_near_poses"] = round(w[0] / (len(near) * src.shape[1]), 1)
                rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--count", action="store_true", help="candidates per point from a -DICPK_SCORE_COUNT build (its timings are not the product's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_bench.json"))
    ap.add_argument("--rows", action="store_true", help="(internal) run the rows in this process and print them")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.rows:
        print("ROWS " + json.dumps(run_rows(a.reps, a.warmup, a.count)))
        return 0
    build.build()
    env = dict(os.environ)
    if a.count:
        if not os.path.exists(COUNT_LIB):  # (built where the compiler is; a GPU visit finds it there)
            os.makedirs(os.path.dirname(COUNT_LIB), exist_ok=True)
            build.build(extra=["-DICPK_SCORE_COUNT"], out=COUNT_LIB)
        env["ICPK_LIB_PATH"] = COUNT_LIB
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows", "--reps", str(a.reps), "--warmup",
                            str(a.warmup)] + (["--count"] if a.count else []), capture_output=True, text=True,
                           timeout=TIMEOUT_S, env=env)
    except subprocess.TimeoutExpired:
        print(f"no result within {TIMEOUT_S} s", file=sys.stderr)
        return 1
    if r.returncode != 0:
        print(f"exit status {r.returncode}\n{r.stderr[-3000:]}", file=sys.stderr)
        return 1
    out = {"reps": a.reps, "warmup": a.warmup, "unit": "ms of host clock around calls that end in a host wait",
           "diagnostic_count_build": bool(a.count),
           "rows": json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ROWS ")][-1][5:])}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
