"""Aggregate frame pairs/s of icpk_align_frames_batch for N depth streams against the sequential frame path.

Tracker settings (threshold 1e-4, 16 iterations at most, resident previous frames), 640 x 480 images with about 30 %
valid pixels.  The sequential figure runs the same N streams one after the other, one context per stream (its previous
frame resident), backproject_pair + align + get_trace per pair: N trackers called in turn.  The batch figure is one
align_frames_batch call per step for all N streams, plus one get_frames_trace per job (MultiSequenceRunner drives
it; with its per-stream Python bookkeeping: with_bookkeeping_pairs_per_s).  Each figure is the median of
`--procs` fresh processes.  Prints one JSON line.

  python tools/bench_multi_tracker.py [--streams 1,4,8,16,32,64] [--steps 8] [--procs 3]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frames(n_streams, steps, rows=480, cols=640, valid=0.30):
    """a pool of room frames along one trajectory; stream s walks it from offset s with its own validity masks"""
    from icp_slam_prototype_amd import synth

    pool_n = steps + 8
    rng = np.random.default_rng(0)
    pool = [synth.render_room_depth(rows, cols, synth.rot_xyz_deg(0, 0.5 * k, 0.1 * k), np.array([0.01 * k, 0, 0.004 * k]),
                                    noise_sigma=0.002, rng=rng) for k in range(pool_n)]
    out = []
    for s in range(n_streams):
        r = np.random.default_rng(100 + s)
        seq = []
        for k in range(steps + 1):
            d = pool[(s + k) % pool_n].copy()
            d[r.random(d.shape) > valid] = 0
            seq.append(d.astype(np.uint16))
        out.append(seq)
    return out


def child(mode, n, steps):
    from icp_slam_prototype_amd import binding, sequence

    par = dict(max_iterations=16, threshold=1e-4)
    st = frames(n, steps)
    with binding.Context(0) as ctx:
        its = 0
        if mode == "seq":
            # the same N streams, one tracker each, advanced one after the other; a context per stream so that each
            # keeps its previous frame resident (icp::Tracker over one Engine each)
            ctxs = [ctx] + [binding.Context(0) for _ in range(n - 1)]
            rs = [sequence.SequenceRunner(c) for c in ctxs]
            for s_, r in enumerate(rs):
                r.step(st[s_][0])
                r.step(st[s_][1])  # (warm-up; from here on the previous frame is resident)
            t0 = time.perf_counter()
            for k in range(2, steps + 1):
                for s_, (c, r) in enumerate(zip(ctxs, rs)):
                    c.backproject_pair(st[s_][k], None, R=r.camera_rotation, t=r.camera_position)
                    T, s, rc = c.align(last_rotation=r.last_rotation, last_translation=r.last_translation, **par)
                    c.get_trace(17)
                    its += s.iterations
            dt = time.perf_counter() - t0
            pairs = (steps - 1) * n
            for c in ctxs[1:]:
                c.close()
        else:
            multi = sequence.MultiSequenceRunner(ctx, n)
            multi.step({s: st[s][0] for s in range(n)})
            multi.step({s: st[s][1] for s in range(n)})  # (warm-up: explicit previous frames, slots allocated)
            inner = [0.0]

            def timed(f):
                def g(*a, **kw):
                    t = time.perf_counter()
                    r = f(*a, **kw)
                    inner[0] += time.perf_counter() - t
                    return r
                return g
            ctx.align_frames_batch, ctx.get_frames_trace = timed(ctx.align_frames_batch), timed(ctx.get_frames_trace)
            t0 = time.perf_counter()
            for k in range(2, steps + 1):
                res = multi.step({s: st[s][k] for s in range(n)})
                its += sum(v["iterations"] for v in res.values())
            dt = time.perf_counter() - t0
            pairs = (steps - 1) * n
            # the library calls alone: MultiSequenceRunner's per-stream Python bookkeeping is left out, as the
            # sequential loop leaves out SequenceRunner's
            print(json.dumps(dict(pairs_per_s=pairs / inner[0], with_bookkeeping_pairs_per_s=pairs / dt,
                                  mean_iterations=its / pairs)))
            return
    print(json.dumps(dict(pairs_per_s=pairs / dt, mean_iterations=its / pairs)))


def run(mode, n, steps):
    out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--child", mode, "--streams", str(n),
                                   "--steps", str(steps)], text=True, timeout=600)
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,4,8,16,32,64")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, int(a.streams), a.steps)
        return
    res = dict(batch={})
    for n in [int(x) for x in a.streams.split(",")]:
        seq = [run("seq", n, a.steps) for _ in range(a.procs)]
        seq_rate = float(np.median([r["pairs_per_s"] for r in seq]))
        b = [run("batch", n, a.steps) for _ in range(a.procs)]
        rate = float(np.median([r["pairs_per_s"] for r in b]))
        res["batch"][n] = dict(pairs_per_s=rate, sequential_pairs_per_s=seq_rate, speedup=rate / seq_rate,
                               mean_iterations=b[0]["mean_iterations"],
                               with_bookkeeping_pairs_per_s=float(np.median([r["with_bookkeeping_pairs_per_s"] for r in b])))
        print(json.dumps({n: res["batch"][n]}), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
