"""TEST INFRASTRUCTURE: the voxel-grid downsampling rule of include/icpk.h (icpk_voxel_downsample, K11) restated in
numpy -- float64 / int64 throughout, the groups from np.unique over the packed voxel keys, the integer sums from
np.add.at.  The GPU tests compare the library against it bit for bit; never imported by the package.

brute_force() states the same rule a third time as a Python loop over the points with a dict of voxels (Python's own
floats and unbounded integers), for test_voxel_host.py to check the numpy version against.
"""
import math

import numpy as np

FIRST, CENTROID = 0, 1
LIMIT = 2 ** 20          # |floor(p / leaf)| beyond it on any axis: the point is dropped
FIX = float(2 ** 30)     # fixed point of the centroid's sums
_RADIX = np.uint64(2 ** 21 + 1)


def voxel_coords(points, leaf):
    """(u, v, kept): u = p / L and v = floor(u) as float64 (3, n); kept (n,) bool -- the points that have a voxel."""
    pts = np.asarray(points, np.float32).reshape(3, -1)
    L = np.float64(np.float32(leaf))
    with np.errstate(all="ignore"):
        u = pts.astype(np.float64) / L
        v = np.floor(u)
        kept = np.isfinite(pts).all(0) & (np.abs(v) <= LIMIT).all(0)  # (a NaN v compares false)
    return u, v, kept


def downsample(points, leaf, mode=CENTROID, normals=None):
    """The rule on a (3, n) float32 cloud (and its (3, n) normals).  Returns dict(points (3, n_out) float32, normals
    (3, n_out) float32 or None, first_index, count (n_out,) int32, out_of_point (n,) int32, n_out, n_dropped)."""
    pts = np.asarray(points, np.float32).reshape(3, -1)
    n = pts.shape[1]
    L = np.float64(np.float32(leaf))
    u, v, kept = voxel_coords(pts, leaf)
    idx = np.flatnonzero(kept)
    b = (v[:, idx].astype(np.int64) + LIMIT).astype(np.uint64)
    key = (b[0] * _RADIX + b[1]) * _RADIX + b[2]  # injective: (2^21 + 1)^3 < 2^64
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    # voxels in the order of their lowest member index
    order = np.argsort(first, kind="stable")
    rank = np.empty(order.size, np.int64)
    rank[order] = np.arange(order.size)
    group = rank[inv]                      # per kept point: its output point
    n_out = order.size
    first_index = idx[first[order]].astype(np.int32)
    count = np.bincount(group, minlength=n_out).astype(np.int32)
    out_of_point = np.full(n, -1, np.int32)
    out_of_point[idx] = group
    nrm = None if normals is None else np.asarray(normals, np.float32).reshape(3, -1)
    if mode == FIRST:
        out = pts[:, first_index].copy()
        out_n = None if nrm is None else nrm[:, first_index].copy()
    else:
        f = u[:, idx] - v[:, idx]
        q = np.rint(f * FIX).astype(np.int64)
        S = np.zeros((3, n_out), np.int64)
        for c in range(3):
            np.add.at(S[c], group, q[c])
        m = count.astype(np.float64)
        out = ((v[:, first_index] + (S.astype(np.float64) / m) / FIX) * L).astype(np.float32)
        out_n = None
        if nrm is not None:
            qn = np.rint(nrm[:, idx].astype(np.float64) * FIX).astype(np.int64)
            N = np.zeros((3, n_out), np.int64)
            for c in range(3):
                np.add.at(N[c], group, qn[c])
            Nd = N.astype(np.float64)
            g = np.sqrt((Nd[0] * Nd[0] + Nd[1] * Nd[1]) + Nd[2] * Nd[2])
            with np.errstate(all="ignore"):
                out_n = np.where(g == 0.0, 0.0, Nd / g).astype(np.float32)
    return dict(points=out, normals=out_n, first_index=first_index, count=count, out_of_point=out_of_point,
                n_out=int(n_out), n_dropped=int(n - idx.size))


def brute_force(points, leaf, mode=CENTROID, normals=None):
    """The same rule, one point after the other (small clouds only).  Same return value as downsample()."""
    pts = np.asarray(points, np.float32).reshape(3, -1)
    nrm = None if normals is None else np.asarray(normals, np.float32).reshape(3, -1)
    n = pts.shape[1]
    L = float(np.float32(leaf))
    voxels = {}  # (vx, vy, vz) -> [output position, first index, members, S[3], N[3]]; dicts keep insertion order
    out_of_point = np.full(n, -1, np.int32)
    dropped = 0
    for i in range(n):
        p = [float(pts[c, i]) for c in range(3)]
        if not all(math.isfinite(x) for x in p):
            dropped += 1
            continue
        u = [x / L for x in p]
        if not all(math.isfinite(x) and abs(math.floor(x)) <= LIMIT for x in u):
            dropped += 1
            continue
        v = tuple(math.floor(x) for x in u)
        e = voxels.setdefault(v, [len(voxels), i, 0, [0, 0, 0], [0, 0, 0]])
        e[2] += 1
        for c in range(3):
            e[3][c] += round((u[c] - v[c]) * FIX)  # (Python rounds ties to even)
            if nrm is not None:
                e[4][c] += round(float(nrm[c, i]) * FIX)
        out_of_point[i] = e[0]
    n_out = len(voxels)
    out = np.zeros((3, n_out), np.float32)
    out_n = None if nrm is None else np.zeros((3, n_out), np.float32)
    first_index = np.zeros(n_out, np.int32)
    count = np.zeros(n_out, np.int32)
    for v, (k, i0, m, S, N) in voxels.items():
        first_index[k], count[k] = i0, m
        if mode == FIRST:
            out[:, k] = pts[:, i0]
            if nrm is not None:
                out_n[:, k] = nrm[:, i0]
            continue
        for c in range(3):
            out[c, k] = np.float32((float(v[c]) + (float(S[c]) / float(m)) / FIX) * L)
        if nrm is not None:
            Nd = [float(x) for x in N]
            g = math.sqrt((Nd[0] * Nd[0] + Nd[1] * Nd[1]) + Nd[2] * Nd[2])
            for c in range(3):
                out_n[c, k] = np.float32(Nd[c] / g) if g != 0.0 else np.float32(0)
    return dict(points=out, normals=out_n, first_index=first_index, count=count, out_of_point=out_of_point,
                n_out=n_out, n_dropped=dropped)


def same(a, b):
    """Two results of downsample() / brute_force() / the library agree bit for bit; returns the first difference."""
    for k in ("n_out", "n_dropped"):
        if a[k] != b[k]:
            return f"{k}: {a[k]} != {b[k]}"
    for k in ("first_index", "count", "out_of_point", "points", "normals"):
        x, y = a.get(k), b.get(k)
        if x is None and y is None:
            continue
        if x is None or y is None:
            return f"{k}: present on one side only"
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.shape != y.shape or x.dtype != y.dtype:
            return f"{k}: {x.dtype}{x.shape} != {y.dtype}{y.shape}"
        if x.tobytes() != y.tobytes():
            bad = np.flatnonzero(x.reshape(-1).view(np.uint32) != y.reshape(-1).view(np.uint32))
            return f"{k}: {bad.size} entries differ, first at {bad[0]}: {x.reshape(-1)[bad[0]]!r} != {y.reshape(-1)[bad[0]]!r}"
    return None
