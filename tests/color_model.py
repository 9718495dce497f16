"""TEST INFRASTRUCTURE: colored ICP as include/icpk.h words it (K17) restated in numpy, operation by operation -- the
integer sums behind the colour gradients over K12's neighbourhoods (tests/normals_model.py), the float64 solve with
the header's association of every product and sum, the 28 sums of the joint step through the canonical reduction tree
(tests/gicp_model.py), the solve by the oracle's solve_p2l and the loop around them.  It never reads the library.  The
GPU tests compare the library against it bit for bit.

numpy evaluates `a * b + c * d` as two rounded products and one rounded sum, never fused, which is what the header
asks for.
"""
import numpy as np

import gicp_model as gm
import normals_model as nm
from robust_model import KdNN

F = 2 ** 15
NP2L = 28
LAMBDA = 0.968
TOL = 2.0 ** -10


def usable_normals(nrm):
    """(n,) bool: the float64 squared length lies in [1 - 2^-10, 1 + 2^-10]"""
    n = np.asarray(nrm, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        return (nn >= 1.0 - TOL) & (nn <= 1.0 + TOL)


def gradient_sums(pts, nrm, inten, radius):
    """(n, 10) int64: m, S_00 S_01 S_02 S_11 S_12 S_22, T_0 T_1 T_2"""
    pts = np.asarray(pts, np.float32).reshape(3, -1)
    nrm = np.asarray(nrm, np.float32).reshape(3, -1)
    inten = np.asarray(inten, np.float32).reshape(-1)
    n = pts.shape[1]
    i, j = nm.neighbour_pairs(pts, radius)
    S = np.zeros((n, 10), np.int64)
    S[:, 0] = np.bincount(i, minlength=n)
    keep = usable_normals(nrm)[i]
    i, j = i[keep], j[keep]
    rd = np.float64(np.float32(radius))
    nv = nrm[:, i].astype(np.float64)
    e = pts[:, j].astype(np.float64) - pts[:, i].astype(np.float64)
    h = (e[0] * nv[0] + e[1] * nv[1]) + e[2] * nv[2]
    u = e - h * nv
    q = np.rint((u / rd) * F).astype(np.int64)
    c = np.rint((inten[j].astype(np.float64) - inten[i].astype(np.float64)) * F).astype(np.int64)
    assert (np.abs(q) <= F + 128).all() and (np.abs(c) <= F).all()
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        np.add.at(S[:, 1 + k], i, q[a] * q[b])
    for a in range(3):
        np.add.at(S[:, 7 + a], i, q[a] * c)
    return S


def gradients_from_sums(S, nrm, radius, min_neighbors):
    """(3, n) float32 gradients from the ten words per point"""
    S = np.asarray(S, np.int64)
    n = np.asarray(nrm, np.float32).reshape(3, -1).astype(np.float64)
    rd = np.float64(np.float32(radius))
    with np.errstate(all="ignore"):
        m = S[:, 0]
        w = m.astype(np.float64) * float(F)
        w2 = w * w
        Sd = S[:, 1:7].astype(np.float64)
        H00 = Sd[:, 0] + (w2 * n[0]) * n[0]
        H01 = Sd[:, 1] + (w2 * n[0]) * n[1]
        H02 = Sd[:, 2] + (w2 * n[0]) * n[2]
        H11 = Sd[:, 3] + (w2 * n[1]) * n[1]
        H12 = Sd[:, 4] + (w2 * n[1]) * n[2]
        H22 = Sd[:, 5] + (w2 * n[2]) * n[2]
        T0, T1, T2 = (S[:, 7 + a].astype(np.float64) for a in range(3))
        K00 = H11 * H22 - H12 * H12
        K01 = H02 * H12 - H01 * H22
        K02 = H01 * H12 - H02 * H11
        K11 = H00 * H22 - H02 * H02
        K12 = H01 * H02 - H00 * H12
        K22 = H00 * H11 - H01 * H01
        det = (H00 * K00 + H01 * K01) + H02 * K02
        inv = 1.0 / det
        g = np.stack([((((K00 * T0 + K01 * T1) + K02 * T2) * inv) / rd),
                      ((((K01 * T0 + K11 * T1) + K12 * T2) * inv) / rd),
                      ((((K02 * T0 + K12 * T1) + K22 * T2) * inv) / rd)]).astype(np.float32)
        ok = (m >= min_neighbors) & usable_normals(nrm) & (det > 0.0) & (det < np.inf) & np.isfinite(g).all(0)
    return np.where(ok[None, :], g, np.float32(0)).astype(np.float32)


def gradients(pts, nrm, inten, radius, min_neighbors=4):
    S = gradient_sums(pts, nrm, inten, radius)
    return gradients_from_sums(S, nrm, radius, min_neighbors), S


def pair_terms(src, tgt, tnrm, grad, tcol, scol, idx, dist, max_dist, lambda_geometric=LAMBDA):
    """(n, 28) float64 terms of every query (zero rows where the pair is not accepted) and the accepted mask"""
    src, tgt = np.asarray(src, np.float32), np.asarray(tgt, np.float32)
    dist = np.asarray(dist, np.float32)
    near = dist < np.float32(max_dist)
    j = np.where(near, idx, 0)
    n = np.asarray(tnrm, np.float32)[:, j].astype(np.float64)
    acc = near & ~((n[0] == 0) & (n[1] == 0) & (n[2] == 0))
    g = np.asarray(grad, np.float32)[:, j].astype(np.float64)
    It = np.asarray(tcol, np.float32)[j].astype(np.float64)
    Is = np.asarray(scol, np.float32).astype(np.float64)
    lg = float(np.float32(lambda_geometric))
    lc = 1.0 - lg
    p = src.astype(np.float64)
    q = tgt[:, j].astype(np.float64)
    with np.errstate(all="ignore"):
        e = p - q
        h = (e[0] * n[0] + e[1] * n[1]) + e[2] * n[2]
        G = [p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2]]
        u = e - h * n
        rc = (It + ((g[0] * u[0] + g[1] * u[1]) + g[2] * u[2])) - Is
        gn = (g[0] * n[0] + g[1] * n[1]) + g[2] * n[2]
        M = g - gn * n
        Cc = [p[1] * M[2] - p[2] * M[1], p[2] * M[0] - p[0] * M[2], p[0] * M[1] - p[1] * M[0], M[0], M[1], M[2]]
        t = [lg * (G[a] * G[b]) + lc * (Cc[a] * Cc[b]) for a in range(6) for b in range(a, 6)]
        t += [lg * (G[a] * h) + lc * (Cc[a] * rc) for a in range(6)]
        t += [dist.astype(np.float64)]
        vals = np.stack(t, axis=1)
    vals[~acc] = 0.0
    return vals, acc


def sums(src, tgt, tnrm, grad, tcol, scol, idx, dist, max_dist, lambda_geometric=LAMBDA):
    """icpk_reduce_colored: (28 float64 sums, accepted count)"""
    vals, acc = pair_terms(src, tgt, tnrm, grad, tcol, scol, idx, dist, max_dist, lambda_geometric)
    return gm.canonical(vals), int(acc.sum())


def sums_p2l(src, tgt, tnrm, idx, dist, max_dist):
    """icpk_reduce_p2l (K5) through the canonical tree: (28 float64 sums, accepted count)"""
    src, tgt = np.asarray(src, np.float32), np.asarray(tgt, np.float32)
    dist = np.asarray(dist, np.float32)
    near = dist < np.float32(max_dist)
    j = np.where(near, idx, 0)
    n = np.asarray(tnrm, np.float32)[:, j].astype(np.float64)
    acc = near & ~((n[0] == 0) & (n[1] == 0) & (n[2] == 0))
    p = src.astype(np.float64)
    q = tgt[:, j].astype(np.float64)
    with np.errstate(all="ignore"):
        J = [p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2]]
        r = ((p[0] - q[0]) * n[0] + (p[1] - q[1]) * n[1]) + (p[2] - q[2]) * n[2]
        t = [J[a] * J[b] for a in range(6) for b in range(a, 6)] + [J[a] * r for a in range(6)] + [dist.astype(np.float64)]
        vals = np.stack(t, axis=1)
    vals[~acc] = 0.0
    return gm.canonical(vals), int(acc.sum())


def align(src, tgt, tnrm, grad, tcol, scol, oracle, iterations=30, max_dist=0.75, lambda_geometric=LAMBDA, min_pairs=3,
          colored=True):
    """Fixed-iteration loop as icpk_align runs it: the motion of every solve applied and recorded in float, the pose
    accumulated in float64.  colored=False: the plain point-to-plane step.  Returns dict(T (4, 4) float64, status
    (0, 1 too few pairs, 2 degenerate), iterations, pairs)."""
    nn = KdNN(np.asarray(tgt, np.float32), oracle)
    cur = np.asarray(src, np.float32).copy()
    Tk = np.eye(4)
    pairs = []
    status = 0
    done = 0
    for _ in range(iterations):
        idx, dist = nn(cur)
        if colored:
            s, cnt = sums(cur, tgt, tnrm, grad, tcol, scol, idx, dist, max_dist, lambda_geometric)
        else:
            s, cnt = sums_p2l(cur, tgt, tnrm, idx, dist, max_dist)
        if cnt < min_pairs:
            status = 1
            break
        pairs.append(cnt)
        R, t, rc = oracle.solve_p2l(s)
        if rc != 0:
            status = 2
            break
        Rf, tf = R.astype(np.float32), t.astype(np.float32)
        cur = oracle.transform_points(cur, Rf, tf)
        step = np.eye(4)
        step[:3, :3], step[:3, 3] = Rf, tf
        Tk = step @ Tk
        done += 1
    idx, dist = nn(cur)
    return dict(T=Tk, status=status, iterations=done, pairs=pairs, final_idx=idx, final_dist=dist, source=cur)


# the flat wall of the issue: the scene, its settings and the bound the host test fixes and the GPU tests reuse
WALL = dict(rows=60, cols=80, relief=0.0, seed=1)
WALL_RADIUS, WALL_MIN_NB, WALL_ITER, WALL_MAX_DIST = 0.035, 4, 30, 0.75
# measured with this model (tests/test_color_host.py prints them): rotation (Frobenius), translation (m)
WALL_MEASURED = (1.8483419573490605e-05, 6.0071094610033886e-05)


def wall_pair(**kw):
    from icp_slam_prototype_amd import synth

    p = synth.textured_wall_pair(**{**WALL, **kw})
    n = p["target"].shape[1]
    p["target_normals"] = np.tile(np.float32([[0], [0], [-1]]), (1, n))  # towards the camera at the origin
    return p


def pose_errors(T, T_true):
    T, T_true = np.asarray(T, np.float64), np.asarray(T_true, np.float64)
    return float(np.linalg.norm(T[:3, :3] - T_true[:3, :3])), float(np.linalg.norm(T[:3, 3] - T_true[:3, 3]))
