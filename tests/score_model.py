"""TEST INFRASTRUCTURE: the pose-scoring rule of include/icpk.h (icpk_score_poses, K15) restated in numpy, operation by
operation -- the float32 transform, the brute-force partner under the (d, j) order, the eleven terms, the canonical
reduction tree (gicp_model.canonical), the metrics and the information matrix.  It never reads the library.  The GPU
tests compare the library's sums, counts and partners against it bit for bit.

numpy evaluates `a * b + c * d` as two rounded products and one rounded sum, never fused; the products of two float32
widened to float64 are exact, so `(r0 * x + r1 * y) + r2 * z` in float64 rounds exactly like the kernel's two fmas.
"""
import numpy as np

from gicp_model import canonical

NSCORE = 11


def transform(src, T):
    """p = fl32(fl32(R s) + t) for (3, n) float32 points and a row-major 4 x 4 float32 pose (row 3 ignored)"""
    src = np.asarray(src, np.float32)
    T = np.asarray(T, np.float32).reshape(4, 4)
    s = src.astype(np.float64)
    R = T[:3, :3].astype(np.float64)
    with np.errstate(all="ignore"):
        rot = [((R[u, 0] * s[0] + R[u, 1] * s[1]) + R[u, 2] * s[2]).astype(np.float32) for u in range(3)]
        return np.stack([rot[u] + T[u, 3] for u in range(3)]).astype(np.float32)


def pair_dist(p, t):
    """(n, m) float32 distances of icp.cpp:606-620 between (3, n) and (3, m) float32 points"""
    with np.errstate(all="ignore"):
        dx = (p[0][:, None] - t[0][None, :]).astype(np.float64)
        dy = (p[1][:, None] - t[1][None, :]).astype(np.float64)
        dz = (p[2][:, None] - t[2][None, :]).astype(np.float64)
        return np.sqrt(((dx * dx + dy * dy) + dz * dz).astype(np.float32))


def partners(p, tgt, max_dist, rows=2048):
    """Per point of p (3, n) float32 the target that minimises (d, j) among those with d < max_dist: (idx (n,) int32,
    -1 for none; dist (n,) float32, +inf for none).  Brute force."""
    p, tgt = np.asarray(p, np.float32), np.asarray(tgt, np.float32)
    n = p.shape[1]
    idx = np.full(n, -1, np.int32)
    dist = np.full(n, np.inf, np.float32)
    md = np.float32(max_dist)
    for a in range(0, n, rows):
        d = pair_dist(p[:, a:a + rows], tgt)
        with np.errstate(all="ignore"):
            d = np.where(d < md, d, np.float32(np.inf))  # (NaN compares false: a non-finite point or target never pairs)
        j = np.argmin(d, axis=1)  # the first minimum: the lowest index on a tie
        dj = d[np.arange(d.shape[0]), j]
        ok = dj < md
        idx[a:a + rows] = np.where(ok, j, -1)
        dist[a:a + rows] = np.where(ok, dj, np.float32(np.inf))
    return idx, dist


def terms(tgt, idx, dist):
    """(n, 11) float64: the eleven terms of every point, a row of +0.0 where it is not an inlier"""
    tgt = np.asarray(tgt, np.float32)
    inl = idx >= 0
    q = tgt[:, np.where(inl, idx, 0)].astype(np.float64)
    dd = np.where(inl, dist, np.float32(0)).astype(np.float64)
    t = np.stack([dd, dd * dd, q[0], q[1], q[2], q[0] * q[0], q[0] * q[1], q[0] * q[2], q[1] * q[1], q[1] * q[2],
                  q[2] * q[2]], axis=1)
    t[~inl] = 0.0
    return t


def score(src, tgt, T, max_dist):
    """One pose (T = None: the points as they stand): dict(sums (11,), inliers, idx, dist)"""
    p = np.asarray(src, np.float32) if T is None else transform(src, T)
    idx, dist = partners(p, tgt, max_dist)
    return dict(sums=canonical(terms(tgt, idx, dist)), inliers=int((idx >= 0).sum()), idx=idx, dist=dist)


def metrics(sums, inliers, n_source):
    """icpk_score_metrics: (fitness, inlier_rmse, mean_dist) float32"""
    n = float(inliers)
    fit = n / float(n_source) if n_source > 0 else 0.0
    rmse = np.sqrt(sums[1] / n) if inliers > 0 else 0.0
    mean = sums[0] / n if inliers > 0 else 0.0
    return np.float32(fit), np.float32(rmse), np.float32(mean)


def information(sums, inliers):
    """icpk_information_matrix: (6, 6) float64 from the sums"""
    sx, sy, sz, xx, xy, xz, yy, yz, zz = (np.float64(v) for v in sums[2:11])
    n = np.float64(inliers)
    u = np.zeros((6, 6))
    u[0, :] = [yy + zz, -xy, -xz, 0.0, -sz, sy]
    u[1, 1:] = [xx + zz, -yz, sz, 0.0, -sx]
    u[2, 2:] = [xx + yy, -sy, sx, 0.0]
    u[3, 3] = u[4, 4] = u[5, 5] = n
    for r in range(6):  # mirrored entry by entry (an addition of the two triangles would turn a -0.0 into +0.0)
        for c in range(r):
            u[r, c] = u[c, r]
    return u


def information_explicit(q):
    """sum G^T G with G = [-[q]x | I] formed point by point in float64, q (3, k)"""
    q = np.asarray(q, np.float64)
    out = np.zeros((6, 6))
    for x, y, z in q.T:
        G = np.zeros((3, 6))
        G[:, :3] = -np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
        G[:, 3:] = np.eye(3)
        out += G.T @ G
    return out
