"""Timing of the Euclidean distance map (icpk_esdf_compute / icpk_esdf_query, K31): the median over --reps calls after
--warmup calls, each call bracketed by HIP events on the context's stream (as tools/bench_tsdf_shift.py).  Prints one
JSON line and writes it to profiles/esdf_bench.json.  No time is asserted anywhere.

Per volume (64^3, 256^3 and 512^3 voxels over the same 5.12 m cube, voxel = 0.08 / 0.02 / 0.01 m, trunc = 4 voxels), one
synthetic 640 x 480 frame of the room fused at the identity pose, then for max_distance = 0.5 and 2.0 m:
  compute_us          icpk_esdf_compute(counts = NULL): the classification, the three passes and the sum, no host wait
  floor_bytes         what the four kernels must move: n (6 + 1) for the classification, n (1 + 4) for x, n 8 for y and z
  floor_us / of_floor floor_bytes over the 6.29 TB/s a float4 copy reaches on the card, and that over compute_us
  query_us            icpk_esdf_query of 65 536 points in and around the volume (uploads, kernel, one download)
  counts, sq_crc32    unknown, free, occupied, far; up to 256^3 the CRC of the sq plane
and at 64^3: host_us, icpk_esdf_host on up to 16 threads (a host clock), the second yardstick.
With --passes every (volume, max_distance) is run once more as a child process under `rocprofv3 --kernel-trace --stats`
(a run of its own: tracing slows the host) and the four kernels' average times come back per pass, each against its own
byte floor: passes = {kernel: {us, floor_us}}."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from icp_slam_prototype_amd import binding, synth

COPY_GBPS = 6290.0
DISTANCES = [0.5, 2.0]
NQUERY = 65536
PASS_BYTES = {"esdf_classify_kernel": 7, "esdf_pass_kernel<0>": 5, "esdf_pass_kernel<1>": 8, "esdf_pass_kernel<2>": 8}


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


def fill(ctx, dim, depth):
    voxel = 5.12 / dim
    ctx.tsdf_create(dims=(dim,) * 3, voxel=voxel, origin=(-2.56, -2.56, 0.4), trunc=4 * voxel, max_weight=255)
    ctx.tsdf_integrate(depth, np.eye(4), fx=float(synth.FX), cx=float(synth.CX))
    return voxel


def room_frame():
    P = np.eye(4)
    return synth.render_room_depth(480, 640, P[:3, :3], P[:3, 3])


def one(dim, dist, reps):
    """the child of --passes: the compute alone, a few times, for the tracer"""
    with binding.Context(0) as ctx:
        fill(ctx, dim, room_frame())
        for _ in range(reps):
            binding.esdf_compute(ctx, max_distance=dist, counts=False)
        binding.esdf_compute(ctx, max_distance=dist)


def traced_passes(dim, dist, reps):
    n = dim ** 3
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "-o", "esdf", "--", sys.executable, os.path.abspath(__file__),
               "--one", str(dim), str(dist), "--reps", str(reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return {"error": r.stderr[-400:]}
        out = {}
        for path in glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name", "")
                for key, per in PASS_BYTES.items():
                    if key in name and "AverageNs" in row:
                        out[key] = {"us": float(row["AverageNs"]) / 1e3, "floor_us": n * per / COPY_GBPS / 1e3}
        return out or {"error": "no kernel statistics came back"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dims", type=int, nargs="*", default=[64, 256, 512])
    ap.add_argument("--passes", action="store_true")
    ap.add_argument("--tag", default="", help="suffix of the output file: a diagnostic build (ICPK_LIB_PATH) keeps its own")
    ap.add_argument("--one", nargs=2, metavar=("DIM", "MAX_DISTANCE"))
    a = ap.parse_args()
    if a.one:
        return one(int(a.one[0]), float(a.one[1]), a.reps)
    depth = room_frame()
    out = {"reps": a.reps, "warmup": a.warmup, "copy_gbps": COPY_GBPS, "n_query": NQUERY, "volumes": []}
    rng = np.random.default_rng(0)
    pts = np.ascontiguousarray(rng.uniform([[-2.7], [-2.7], [0.3]], [[2.7], [2.7], [5.6]], (3, NQUERY)).astype(np.float32))
    with binding.Context(0) as ctx:
        for dim in a.dims:
            voxel = fill(ctx, dim, depth)
            n = dim ** 3
            r = {"dims": [dim] * 3, "voxel": voxel, "floor_bytes": n * sum(PASS_BYTES.values()), "runs": []}
            r["floor_us"] = r["floor_bytes"] / COPY_GBPS / 1e3
            for dist in DISTANCES:
                e = {"max_distance": dist, "R": int(np.floor(float(np.float32(dist)) / float(np.float32(voxel))))}
                e["counts"] = [int(v) for v in binding.esdf_compute(ctx, max_distance=dist)]
                if dim <= 256:  # (what two builds must agree on before their times are compared)
                    e["sq_crc32"] = zlib.crc32(binding.esdf_get(ctx, cls=False, dist=False)[0].tobytes())
                e["compute_us"] = timed(ctx, lambda: binding.esdf_compute(ctx, max_distance=dist, counts=False), a.warmup, a.reps)
                e["of_floor"] = r["floor_us"] / e["compute_us"]
                e["query_us"] = timed(ctx, lambda: binding.esdf_query(ctx, pts), a.warmup, a.reps)
                if dim == 64:
                    tsdf, weight, _ = ctx.tsdf_get()
                    p, _ = binding.tsdf_get_params(ctx)
                    t0 = time.perf_counter()
                    binding.esdf_host(p, tsdf, weight, max_distance=dist)
                    e["host_us"] = 1e6 * (time.perf_counter() - t0)
                r["runs"].append(e)
            out["volumes"].append(r)
            ctx.tsdf_release()
    if a.passes:
        for r in out["volumes"]:
            for e in r["runs"]:
                e["passes"] = traced_passes(r["dims"][0], e["max_distance"], 3)
    line = json.dumps(out)
    print(line)
    with open(os.path.join(ROOT, "profiles", f"esdf_bench{a.tag}.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
