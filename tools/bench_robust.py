"""Cost of robust alignment (include/icpk.h, icpk_set_robust): microseconds per iteration of the device
loop, 20 fixed iterations, plain against Huber-median, Tukey-median and trim 0.8 -- Kabsch on the 640 x 480 30 % pair,
point-to-plane on the Kinect-v2 pair.  Prints one JSON line.

    python tools/bench_robust.py [--reps 30] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from icp_slam_prototype_amd import binding, build, synth  # noqa: E402

SETTINGS = {
    "plain": None,
    "huber_median": dict(kernel=binding.ROBUST_HUBER, scale=1.0, scale_mode=binding.SCALE_MEDIAN, trim=1.0),
    "tukey_median": dict(kernel=binding.ROBUST_TUKEY, scale=4.685, scale_mode=binding.SCALE_MEDIAN, trim=1.0),
    "trim_0.8": dict(kernel=binding.ROBUST_NONE, scale=1.0, scale_mode=binding.SCALE_FIXED, trim=0.8),
}
ITERS = 20


def time_setting(ctx, cfg, params, reps, warmup):
    ctx.set_robust(None) if cfg is None else ctx.set_robust(**cfg)
    for _ in range(warmup):
        ctx.align(params)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        _, st, rc = ctx.align(params)
        t.append(time.perf_counter() - t0)
        assert rc == 0 and st.iterations == ITERS, (rc, st.iterations)
    t.sort()
    return 1e6 * t[len(t) // 2] / ITERS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    build.build()
    out = {"metric": "us_per_iteration_median", "iterations": ITERS}
    with binding.Context(0) as ctx:
        p = synth.kinect_pair()
        ctx.set_target(p["target"])
        ctx.set_source(p["source"])
        params = binding.default_params(solve=binding.SOLVE_KABSCH, max_iterations=ITERS, fixed_iterations=1)
        out["kabsch_kinect640x480_30pct"] = {k: round(time_setting(ctx, cfg, params, a.reps, a.warmup), 2)
                                             for k, cfg in SETTINGS.items()}
        w = synth.kinect_pair(424, 512, valid=1.0, seed=2, fx=synth.K2_FX, cx=synth.K2_CX)
        ctx.backproject_with_normals(w["depth_tgt"], binding.NORMALS_CROSS, offset=[5, 5, 5], fx=float(synth.K2_FX),
                                     cx=float(synth.K2_CX))
        ctx.backproject(w["depth_src"], which=0, offset=[5, 5, 5], fx=float(synth.K2_FX), cx=float(synth.K2_CX))
        params = binding.default_params(solve=binding.SOLVE_POINT_TO_PLANE, max_iterations=ITERS, fixed_iterations=1,
                                        max_nn_dist=0.3)
        out["p2l_kinect_v2_512x424"] = {k: round(time_setting(ctx, cfg, params, a.reps, a.warmup), 2)
                                        for k, cfg in SETTINGS.items()}
        ctx.set_robust(None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
