"""Cost of pose-graph optimisation on the device (icpk_pose_graph_optimize) on a synthetic trajectory:

  a closed path of n nodes (a ring of radius n / 50 m with a slow vertical wave), odometry edges i + 1 -> i, and
  n / 20 loop closures (5 % of the nodes) between seeded random pairs (s, t) at least n / 8 nodes apart along the
  path, every fifth of them false (the true relative pose displaced by N(0, 0.3 rad), N(0, 0.3 m)); measurements
  perturbed by N(0, 0.01 rad), N(0, 0.02 m); the initial poses are the chained odometry; mu = 2 with pruning.

for n = 1 000 and n = 20 000: the wall time of one Context.pose_graph_optimize call (edge marshalling in Python
excluded: the ctypes edge array is built once) and of its LM iterations (the call's time over their number), beside
scipy.optimize.least_squares (trf, sparse Jacobian pattern, the same whitened residual) on the 1 000-node graph.  Host
clock around calls that end in a host wait; --warmup calls first; median, minimum and maximum of --reps (>= 5).
Prints one JSON line and writes it to --out.

    python tools/posegraph_bench.py [--reps 5] [--warmup 1] [--no-scipy] [--out profiles/posegraph_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from icp_slam_prototype_amd import binding  # noqa: E402


# ---- the rule of include/icpk.h written the ordinary way (numpy products, libm): for the generator and for scipy ------
def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def exp_pose(d):
    """Exp(d) = [Rodrigues(w) | v]"""
    w, th = np.asarray(d[:3], np.float64), float(np.linalg.norm(d[:3]))
    a, b = (np.sin(th) / th, (1.0 - np.cos(th)) / (th * th)) if th > 1e-8 else (1.0, 0.5)
    D = np.eye(4)
    D[:3, :3] = np.eye(3) + a * skew(w) + b * (skew(w) @ skew(w))
    D[:3, 3] = d[3:]
    return D


def inv_pose(P):
    Q = np.eye(4)
    Q[:3, :3] = P[:3, :3].T
    Q[:3, 3] = -P[:3, :3].T @ P[:3, 3]
    return Q


def residual(Ps, Pt, T):
    """r = (rotation vector of R_E, t_E), E = P_t^-1 P_s T^-1"""
    E = inv_pose(Pt) @ Ps @ inv_pose(T)
    R = E[:3, :3]
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = float(np.linalg.norm(v)), 0.5 * (float(np.trace(R)) - 1.0)
    return np.concatenate([v * (np.arctan2(s, c) / s) if s > 1e-12 else v, E[:3, 3]])


def trajectory(n, seed=1):
    rng = np.random.default_rng(seed)
    radius = n / 50.0
    truth = np.zeros((n, 4, 4))
    for i in range(n):
        a = 2.0 * np.pi * i / n
        yaw = a + np.pi / 2.0
        truth[i] = np.eye(4)
        truth[i, :3, :3] = [[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]]
        truth[i, :3, 3] = [radius * np.cos(a), radius * np.sin(a), 0.2 * np.sin(8.0 * a)]

    def info():
        L = np.zeros((6, 6))
        for q in rng.normal(0.0, 1.5, (40, 3)):  # sum G^T G, G = [-[q]x | I]: icpk_information_matrix's form
            G = np.hstack([-skew(q), np.eye(3)])
            L += G.T @ G
        return L

    def measured(s, t, offset=None):
        T = inv_pose(truth[t]) @ truth[s]
        if offset is not None:
            T = exp_pose(offset) @ T
        return exp_pose(np.concatenate([rng.normal(0.0, 0.01, 3), rng.normal(0.0, 0.02, 3)])) @ T

    edges = [(i + 1, i, measured(i + 1, i), info(), False) for i in range(n - 1)]
    n_closures = max(1, n // 20)
    for k in range(n_closures):
        s = int(rng.integers(n // 8, n))
        t = int(rng.integers(0, max(1, s - n // 8)))
        false = k % 5 == 4
        off = np.concatenate([rng.normal(0.0, 0.3, 3), rng.normal(0.0, 0.3, 3)]) if false else None
        edges.append((s, t, measured(s, t, off), info(), True))
    poses = np.zeros_like(truth)
    poses[0] = truth[0]
    for i in range(n - 1):
        poses[i + 1] = poses[i] @ edges[i][2]
    return truth, poses, edges


def stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1], n=len(v))


def device_rows(ctx, poses, edges, reps, warmup, mu):
    dp = C.POINTER(C.c_double)
    arr = binding.pg_edges(edges)
    p = binding.default_pg_params(preference_loop_closure=mu, flags=binding.PG_PRUNE)
    n, m = len(poses), len(edges)
    times, res = [], binding.PgResult()
    for k in range(warmup + reps):
        P = np.array(poses, np.float64, order="C")
        t0 = time.perf_counter()
        rc = ctx._lib.icpk_pose_graph_optimize(ctx._h, n, P.ctypes.data_as(dp), m, arr, C.byref(p), C.byref(res), None,
                                               None, None)
        dt = time.perf_counter() - t0
        if rc < 0:
            raise RuntimeError(f"icpk_pose_graph_optimize: {rc}")
        if k >= warmup:
            times.append(dt * 1e3)
    return dict(optimize_ms=stats(times), per_lm_iteration_ms=stats([t / max(res.iterations, 1) for t in times]),
                iterations=res.iterations, accepted=res.accepted, pcg_iterations=res.pcg_iterations, n_pruned=res.n_pruned,
                initial_cost=res.initial_cost, final_cost=res.final_cost, status=rc), P


def scipy_row(poses, edges, mu):
    from scipy.optimize import least_squares
    from scipy.sparse import lil_matrix

    n = len(poses)
    chol = [np.linalg.cholesky(e[3]) for e in edges]
    rows = sum(7 if (e[4] and mu > 0) else 6 for e in edges)
    pat = lil_matrix((rows, 6 * (n - 1)), dtype=np.int8)
    r0 = 0
    for e in edges:
        k = 7 if (e[4] and mu > 0) else 6
        for node in (e[0], e[1]):
            if node > 0:
                pat[r0:r0 + k, 6 * (node - 1):6 * node] = 1
        r0 += k

    def fun(x):
        P = np.array(poses)
        for i in range(1, n):
            P[i] = exp_pose(x[6 * (i - 1):6 * i]) @ poses[i]
        out = []
        for (s, t, T, info, unc), Cc in zip(edges, chol):
            w = Cc.T @ residual(P[s], P[t], T)
            if unc and mu > 0:
                sl = mu / (mu + float(w @ w))
                out.append(sl * w)
                out.append([np.sqrt(mu) * (sl - 1.0)])
            else:
                out.append(w)
        return np.concatenate(out)

    t0 = time.perf_counter()
    res = least_squares(fun, np.zeros(6 * (n - 1)), method="trf", jac_sparsity=pat, ftol=1e-9, xtol=1e-10, gtol=1e-10)
    return dict(wall_ms=(time.perf_counter() - t0) * 1e3, nfev=int(res.nfev), cost=2.0 * float(res.cost),
                note="no pruning pass; finite-difference Jacobian over the sparsity pattern; one run")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posegraph_bench.json"))
    a = ap.parse_args()
    mu = 2.0
    out = dict(tool="posegraph_bench", reps=a.reps, warmup=a.warmup, mu=mu, graphs=[])
    with binding.Context(0) as ctx:
        for n in (1000, 20000):
            truth, poses, edges = trajectory(n)
            row, P = device_rows(ctx, poses, edges, max(a.reps, 5), a.warmup, mu)
            row.update(n_nodes=n, n_edges=len(edges), error_before=float(np.abs(poses - truth).max()),
                       error_after=float(np.abs(P - truth).max()))
            if n == 1000 and not a.no_scipy:
                row["scipy"] = scipy_row(poses, edges, mu)
            out["graphs"].append(row)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
