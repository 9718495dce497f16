"""TEST INFRASTRUCTURE: the rule of icpk_remove_outliers (include/icpk.h, K13) restated in numpy -- the k nearest
neighbours from a k-d tree's candidates (k plus a margin) re-evaluated with the exact pair distance, the sums S1 / S2
through a restatement of the canonical reduction tree, the radius filter's counts from normals_model's neighbourhoods.
The GPU tests compare the library against it bit for bit.  Never imported by the package.

brute_force() states the same rule a second time, point by point over all n^2 pairs in a literal double loop with no
spatial index, for test_filter_host.py to check the numpy version against.
"""
import numpy as np
from scipy.spatial import cKDTree

import normals_model as nm

STATISTICAL, RADIUS = 0, 1
MAX_K = 64
RED_THREADS, RED_MAX_BLOCKS = 256, 256

pair_dist = nm.pair_dist


def _tree_256(v):
    """(..., 256) float64 -> (...): the 64-lane xor butterfly (32, 16, .., 1) per wave, then ((w0 + w1) + w2) + w3"""
    w = v.reshape(v.shape[:-1] + (4, 64))
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lanes ^ m]
    w = w[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def canonical_sum(v):
    """The canonical tree of include/icpk.h over the float64 elements v[0 .. n): B = clamp(ceil(n / 256), 1, 256)
    blocks, lane g adds elements g, g + 256 B, ... in order, the tree above per block, and once more over the B block
    sums padded to 256 slots with +0.0.  (A lane starts from +0.0 and no element here is -0.0, so the padding of the
    last pass with +0.0 adds nothing.)"""
    v = np.asarray(v, np.float64)
    assert not np.signbit(v).any()
    n = v.size
    B = min(max(-(-n // RED_THREADS), 1), RED_MAX_BLOCKS)
    P = B * RED_THREADS
    L = max(-(-n // P), 1)
    pad = np.zeros(L * P, np.float64)
    pad[:n] = v
    rows = pad.reshape(L, P)
    acc = np.zeros(P, np.float64)
    for r in range(L):
        acc = acc + rows[r]
    slots = np.zeros(RED_MAX_BLOCKS, np.float64)
    slots[:B] = _tree_256(acc.reshape(B, RED_THREADS))
    return float(_tree_256(slots))


def knn_stats(pts, k, margin=8):
    """mean_i (float64), kth_i (float32) of every point and N; a non-finite point reads 0, 0.

    Candidates: the k + 1 + margin nearest of a float64 k-d tree (the point itself among them), their distances
    re-evaluated by the rule.  The margin was enough for point i when the tree's last candidate is further, in real
    terms, than the rule's k'-th distance by more than the float rounding: every point the tree did not return is at
    least as far as that last one, and the rule's distance is below the real one by less than 2^-19 of it -- so none of
    them can be among the k' smallest.  Where that does not hold (duplicates, dense ties) the candidates are doubled
    until it does or until they are the whole cloud.  100 % of the points pass one or the other: nothing is skipped."""
    pts = np.asarray(pts, np.float32).reshape(3, -1)
    n = pts.shape[1]
    assert 1 <= k <= MAX_K
    mean = np.zeros(n, np.float64)
    kth = np.zeros(n, np.float32)
    fin = np.flatnonzero(np.isfinite(pts).all(0))
    N = fin.size
    kp = min(k, N - 1)
    if kp <= 0:
        return mean, kth, N
    p = pts[:, fin]
    tree = cKDTree(p.astype(np.float64).T)
    todo = np.arange(N)
    kq = min(k + 1 + margin, N)
    while todo.size:
        again = []
        for lo in range(0, todo.size, 32768):
            sel = todo[lo:lo + 32768]
            r, c = tree.query(p[:, sel].astype(np.float64).T, k=kq)
            r, c = r.reshape(sel.size, kq), c.reshape(sel.size, kq)
            d = pair_dist(p[:, sel][:, :, None], p[:, c])
            d = np.where(c == sel[:, None], np.float32(np.inf), d.astype(np.float32))  # not a neighbour of itself, by index
            d.sort(axis=1)
            kd = d[:, kp - 1]
            ok = (r[:, -1] * (1.0 - 1e-5) > kd.astype(np.float64)) if kq < N else np.ones(sel.size, bool)
            ok &= np.isfinite(kd)
            assert ok.all() or kq < N
            D = np.zeros(sel.size, np.float64)
            for col in range(kp):
                D = D + d[:, col].astype(np.float64)
            good = sel[ok]
            mean[fin[good]] = D[ok] / np.float64(kp)
            kth[fin[good]] = kd[ok]
            again.append(sel[~ok])
        todo = np.concatenate(again) if again else np.zeros(0, np.int64)
        kq = min(2 * kq, N)
    return mean, kth, N


def radius_counts(pts, radius):
    """m_i of K12's neighbourhood (i itself and duplicates included); 0 for a non-finite point"""
    pts = np.asarray(pts, np.float32).reshape(3, -1)
    i, _ = nm.neighbour_pairs(pts, radius)
    return np.bincount(i, minlength=pts.shape[1]).astype(np.int64)


def threshold(mean, N, std_ratio):
    """summary (N, mu, sigma, T) of the rule from the mean_i in index order (dropped points: +0.0)"""
    if N == 0:
        return np.zeros(4, np.float64)
    S1, S2 = np.float64(canonical_sum(mean)), np.float64(canonical_sum(mean * mean))
    Nd = np.float64(N)
    mu = S1 / Nd
    var = (S2 - S1 * S1 / Nd) / (Nd - np.float64(1.0)) if N >= 2 else np.float64(0.0)
    var = var if var > 0.0 else np.float64(0.0)
    sigma = np.sqrt(var)
    return np.array([Nd, mu, sigma, mu + np.float64(np.float32(std_ratio)) * sigma], np.float64)


def _finish(pts, value, kth, keep, summary, normals):
    fin = np.isfinite(pts).all(0)
    keep = keep & fin
    out_index = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    out = dict(value=value, kth=kth, keep=keep, out_index=out_index, summary=summary, n_out=int(keep.sum()),
               n_dropped=int((~fin).sum()), points=pts[:, keep])
    if normals is not None:
        out["normals"] = np.asarray(normals, np.float32).reshape(3, -1)[:, keep]
    return out


def remove_outliers(pts, kind=STATISTICAL, k=16, std_ratio=2.0, radius=0.05, min_neighbors=5, normals=None):
    """dict(value, kth, keep, out_index, summary, n_out, n_dropped, points[, normals]) of the rule"""
    pts = np.asarray(pts, np.float32).reshape(3, -1)
    if kind == STATISTICAL:
        mean, kth, N = knn_stats(pts, k)
        summary = threshold(mean, N, std_ratio)
        return _finish(pts, mean, kth, mean <= summary[3], summary, normals)
    m = radius_counts(pts, radius)
    N = int(np.isfinite(pts).all(0).sum())
    summary = np.array([N, 0.0, 0.0, min_neighbors], np.float64)
    return _finish(pts, m.astype(np.float64), None, m >= min_neighbors, summary, normals)


def brute_force(pts, kind=STATISTICAL, k=16, std_ratio=2.0, radius=0.05, min_neighbors=5):
    """The rule once more as a literal double loop over all pairs (small clouds only)."""
    pts = np.asarray(pts, np.float32).reshape(3, -1)
    n = pts.shape[1]
    x, y, z = (pts[c] for c in range(3))
    fin = [bool(np.isfinite(x[i]) and np.isfinite(y[i]) and np.isfinite(z[i])) for i in range(n)]
    N = sum(fin)
    value = np.zeros(n, np.float64)
    kth = np.zeros(n, np.float32)
    r = np.float32(radius)
    with np.errstate(all="ignore"):
        for i in range(n):
            if not fin[i]:
                continue
            ds = []
            m = 0
            for j in range(n):
                if not fin[j]:
                    continue
                dx, dy, dz = np.float64(x[i] - x[j]), np.float64(y[i] - y[j]), np.float64(z[i] - z[j])
                d = np.sqrt(np.float32((dx * dx + dy * dy) + dz * dz))
                if d <= r:
                    m += 1
                if j != i:
                    ds.append((d, j))
            if kind == RADIUS:
                value[i] = m
                continue
            ds.sort()
            kp = min(k, N - 1)
            D = np.float64(0.0)
            for d, _ in ds[:kp]:
                D = D + np.float64(d)
            if kp > 0:
                value[i] = D / np.float64(kp)
                kth[i] = ds[kp - 1][0]
    if kind == RADIUS:
        keep = np.array([fin[i] and value[i] >= min_neighbors for i in range(n)], bool).reshape(n)
        return _finish(pts, value, None, keep, np.array([N, 0.0, 0.0, min_neighbors], np.float64), None)
    summary = threshold(value, N, std_ratio)
    keep = np.array([fin[i] and value[i] <= summary[3] for i in range(n)], bool).reshape(n)
    return _finish(pts, value, kth, keep, summary, None)


def same(a, b):
    """None if two results agree bit for bit, else the name of the first field that differs"""
    for key in ("value", "kth", "keep", "out_index", "summary", "points"):
        u, v = a[key], b[key]
        if (u is None) != (v is None):
            return key
        if u is None:
            continue
        u, v = np.ascontiguousarray(u), np.ascontiguousarray(v)
        if u.shape != v.shape or u.dtype != v.dtype:
            return key + " (shape / type)"
        w = {4: np.uint32, 8: np.uint64, 1: np.uint8}[u.dtype.itemsize]
        if not np.array_equal(u.view(w), v.view(w)):
            return key
    if (a["n_out"], a["n_dropped"]) != (b["n_out"], b["n_dropped"]):
        return "counts"
    return None


def with_strays(cloud, share=0.02, seed=7):
    """cloud plus share * n extra points drawn uniformly in its bounding box (default_rng(seed), rounded to float),
    appended; returns (points, is_stray)"""
    cloud = np.asarray(cloud, np.float32).reshape(3, -1)
    n = cloud.shape[1]
    m = int(round(share * n))
    lo, hi = cloud.min(axis=1).astype(np.float64), cloud.max(axis=1).astype(np.float64)
    s = np.random.default_rng(seed).uniform(lo[:, None], hi[:, None], (3, m)).astype(np.float32)
    stray = np.zeros(n + m, bool)
    stray[n:] = True
    return np.concatenate([cloud, s], axis=1), stray
