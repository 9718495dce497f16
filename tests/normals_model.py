"""TEST INFRASTRUCTURE: the rule of icpk_estimate_target_normals (include/icpk.h, K12) restated in numpy -- the
neighbourhoods from a k-d tree's superset filtered by the exact pair distance, the moments as exact integers, the
eigen-solve by numpy.linalg.eigh.  The GPU tests compare the library against it: the counts and moments bit for bit, the
normals and curvatures within derived bounds.  Never imported by the package.

brute_force() states the same rule a second time, point by point over all n^2 pairs with Python's own unbounded
integers and no spatial index, for test_normals_host.py to check the numpy version against.
"""
import numpy as np
from scipy.spatial import cKDTree

F = 2 ** 15
LINE = 2.0 ** -20   # l1 <= LINE * l2: the neighbourhood is a line or a point


def pair_dist(a, b):
    """icp.cpp:606-620 on (3, k) float32 arrays: float differences, float64 sum of squares, narrowed, float sqrt."""
    with np.errstate(all="ignore"):
        d = (a - b).astype(np.float32).astype(np.float64)
        s = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        return np.sqrt(s.astype(np.float32))


def neighbour_pairs(pts, radius):
    """(i, j) of every ordered pair with d(i, j) <= r, i == j included, sorted by nothing in particular."""
    pts = np.asarray(pts, np.float32).reshape(3, -1)
    r = np.float32(radius)
    fin = np.flatnonzero(np.isfinite(pts).all(0))
    if fin.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    p64 = pts[:, fin].astype(np.float64).T
    # superset: the rule's d <= r implies a real distance <= r (1 + 2^-19) + 2^-74
    cand = cKDTree(p64).query_pairs(float(r) * (1.0 + 1e-5) + 1e-44, output_type="ndarray")
    a, b = fin[cand[:, 0]], fin[cand[:, 1]]
    keep = pair_dist(pts[:, a], pts[:, b]) <= r   # (symmetric: the differences only change sign)
    a, b = a[keep], b[keep]
    return np.concatenate([a, b, fin]), np.concatenate([b, a, fin])


def moments(pts, radius):
    """(n, 10) int64: m, S_x S_y S_z, S_xx S_xy S_xz S_yy S_yz S_zz."""
    pts = np.asarray(pts, np.float32).reshape(3, -1)
    n = pts.shape[1]
    i, j = neighbour_pairs(pts, radius)
    rd = np.float64(np.float32(radius))
    u = (pts[:, j].astype(np.float64) - pts[:, i].astype(np.float64)) / rd
    q = np.rint(u * F)
    assert (np.abs(q) <= F + 1).all()
    M = np.zeros((n, 10), np.int64)
    M[:, 0] = np.bincount(i, minlength=n)
    # float64 sums of integers are exact while they stay below 2^53
    assert int(M[:, 0].max(initial=0)) * (F + 1) ** 2 < 2 ** 53
    for k in range(3):
        M[:, 1 + k] = np.bincount(i, weights=q[k], minlength=n).astype(np.int64)
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        M[:, 4 + k] = np.bincount(i, weights=q[a] * q[b], minlength=n).astype(np.int64)
    return M


def covariance(M):
    """(n, 3, 3) float64 from the moments, as the rule words it; NaN where m == 0."""
    M = np.asarray(M, np.int64)
    with np.errstate(all="ignore"):
        m = M[:, 0].astype(np.float64)
        S = M[:, 1:4].astype(np.float64)
        C = np.empty((M.shape[0], 3, 3), np.float64)
        for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            C[:, a, b] = C[:, b, a] = M[:, 4 + k].astype(np.float64) - S[:, a] * S[:, b] / m
    return C


def normals_from_moments(pts, M, min_neighbors=5, viewpoint=None):
    """The rest of the rule.  dict(normals (3, n) float32, curvature (n,) float32, valid (n,) bool, lam (n, 3) float64
    ascending, e0 (n, 3) float64 oriented, s (n,) float64 (NaN without a viewpoint), C (n, 3, 3))."""
    pts = np.asarray(pts, np.float32).reshape(3, -1)
    n = pts.shape[1]
    C = covariance(M)
    okC = np.isfinite(C).all((1, 2))
    Cs = np.where(okC[:, None, None], C, np.eye(3))
    lam, vec = np.linalg.eigh(Cs) if n else (np.zeros((0, 3)), np.zeros((0, 3, 3)))
    e0 = vec[:, :, 0].copy()
    with np.errstate(all="ignore"):
        valid = okC & (M[:, 0] >= min_neighbors) & ~(lam[:, 1] <= LINE * lam[:, 2])
        curv = lam[:, 0] / lam.sum(1)
        valid &= np.isfinite(curv)
        s = np.full(n, np.nan)
        if viewpoint is not None:
            v = np.asarray(viewpoint, np.float32).astype(np.float64)
            s = (e0 * (v[None, :] - pts.T.astype(np.float64))).sum(1)
        big = e0[np.arange(n), np.argmax(np.abs(e0), axis=1)]   # (argmax: the lowest axis on a tie)
        flip = np.where((s < 0) | (s > 0), s < 0, big < 0)
    e0[flip] *= -1.0
    nrm = np.where(valid[None, :], e0.T, 0.0).astype(np.float32)
    return dict(normals=nrm, curvature=np.where(valid, curv, 0.0).astype(np.float32), valid=valid, lam=lam, e0=e0, s=s, C=C)


def estimate(pts, radius, min_neighbors=5, viewpoint=None):
    """The whole rule: normals_from_moments' dict plus count (n,) int32 and moments (n, 10) int64."""
    M = moments(pts, radius)
    out = normals_from_moments(pts, M, min_neighbors, viewpoint)
    out["moments"] = M
    out["count"] = M[:, 0].astype(np.int32)
    out["n_valid"] = int(out["valid"].sum())
    return out


def brute_force(pts, radius):
    """The counts and moments once more: every point against every point, Python integers.  (n, 10) list of ints."""
    pts = np.asarray(pts, np.float32).reshape(3, -1)
    n = pts.shape[1]
    r32 = np.float32(radius)
    r = float(r32)
    out = []
    for i in range(n):
        row = [0] * 10
        pi = pts[:, i]
        for j in range(n):
            pj = pts[:, j]
            with np.errstate(all="ignore"):
                dx, dy, dz = (np.float32(pi[c] - pj[c]) for c in range(3))
                s = float(dx) * float(dx) + float(dy) * float(dy) + float(dz) * float(dz)
                d = np.sqrt(np.float32(s))
            if not d <= r32:   # (NaN and inf compare false)
                continue
            q = [int(np.rint((float(pj[c]) - float(pi[c])) / r * F)) for c in range(3)]
            row[0] += 1
            for c in range(3):
                row[1 + c] += q[c]
            for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                row[4 + k] += q[a] * q[b]
        out.append(row)
    return out
