"""THE DISTANCE RULE and THE QUERY RULE of include/icpk.h (K31) restated in numpy.

The distance rule is an integer rule, so any exact algorithm is a model of it.  Two are here, and they share no code
with each other or with csrc/esdf_rule.h:

  brute      the definition itself: for every voxel the minimum of |v - u|^2 over every voxel u of the other kind, in
             chunks; O(N^2), for the cases where that is affordable (the host test runs it on every case of up to
             BRUTE_MAX_PAIRS pairs).
  separable  three passes of the FULL one-dimensional transform, out[j] = min over ALL j' of in[j'] + (j - j')^2, by
             broadcasting a (len, len) table over the lines: exact for any distance (no window, no radius), O(N len).
             It is what the larger cases (the room) are held to; the host test holds it to `brute` on the others.

Both give the unbounded squared distances; `signed_sq` applies the radius: beyond R^2 the value is FAR.  The query rule
is restated elementwise in float32, one rounding per operation in the order the header writes them; the cell and the
trilinear value are tsdf_raycast_model's and the gradient is sdf_track_model's."""
import numpy as np

import sdf_track_model
import tsdf_raycast_model as rm

F = np.float32
FAR = 2 ** 31 - 1
INF = 2 ** 40  # "no such voxel" in the unbounded int64 distances
UNKNOWN, FREE, OCCUPIED = 0, 1, 2
UNKNOWN_OCCUPIED = 1
Q_FAR, Q_UNKNOWN, Q_OUTSIDE = 1, 2, 0x80
BRUTE_MAX_PAIRS = 4e8


def radius(max_distance, voxel):
    """rule 0: floor in double of the float parameters"""
    return int(np.floor(float(F(max_distance)) / float(F(voxel))))


def classes(tsdf, weight, min_weight=1):
    """rule 1, over (dz, dy, dx) planes"""
    known = np.asarray(weight).astype(np.int64) >= min_weight
    return np.where(~known, UNKNOWN, np.where(np.asarray(tsdf, F) < 0, OCCUPIED, FREE)).astype(np.uint8)


def obstacles(cls, flags=0):
    """rule 2"""
    return cls != FREE if flags & UNKNOWN_OCCUPIED else cls == OCCUPIED


def _nearest_brute(targets, sites):
    """min over the rows of `sites` of the squared distance to every row of `targets` (int64 (n, 3) index arrays)"""
    out = np.full(len(targets), INF, np.int64)
    if len(sites) == 0 or len(targets) == 0:
        return out
    step = max(1, int(2e7 // len(sites)))
    s = sites.astype(np.int32)
    for lo in range(0, len(targets), step):
        t = targets[lo:lo + step].astype(np.int32)
        d = np.zeros((len(t), len(s)), np.int32)
        for a in range(3):
            diff = t[:, a, None] - s[None, :, a]
            d += diff * diff  # (dims of a case < 2^15: no overflow)
        out[lo:lo + step] = d.min(1)
    return out


def brute(in_O):
    """The unbounded signed squared distances by the definition: + to the nearest voxel of O outside it, - to the
    nearest voxel outside O inside it, INF where there is none."""
    idx = np.stack(np.nonzero(np.ones(in_O.shape, bool)), 1)  # (z, y, x) rows in linear order
    flat = in_O.reshape(-1)
    inside, outside = idx[flat], idx[~flat]
    out = np.empty(flat.size, np.int64)
    out[~flat] = _nearest_brute(outside, inside)
    out[flat] = -_nearest_brute(inside, outside)
    return out.reshape(in_O.shape)


def _transform(sites):
    """the exact squared Euclidean distance transform to the True voxels of `sites`, unbounded (INF: none)"""
    d = np.where(sites, 0, INF).astype(np.int64)
    for axis in range(3):
        n = d.shape[axis]
        j = np.arange(n, dtype=np.int64)
        table = (j[:, None] - j[None, :]) ** 2  # [j, j']
        lines = np.moveaxis(d, axis, -1)        # (..., j')
        out = np.empty_like(lines)
        for k in range(n):                      # out[..., k] = min over j' of lines[..., j'] + (k - j')^2
            out[..., k] = (lines + table[k]).min(-1)
        d = np.minimum(np.moveaxis(out, -1, axis), INF)
    return d


def separable(in_O):
    """brute(in_O) by three full one-dimensional passes"""
    return np.where(in_O, -_transform(~in_O), _transform(in_O))


def signed_sq(unbounded, R):
    """rule 3: the unbounded distances through the radius"""
    mag = np.abs(unbounded)
    q = np.where(mag <= R * R, mag, FAR)
    return np.where(unbounded < 0, -q, q).astype(np.int32)


def metric(q, R, voxel):
    """rule 4, float32, one rounding per operation"""
    mag = np.abs(q.astype(np.int64))
    s = np.where(mag == FAR, F(R + 1), np.sqrt(np.where(mag == FAR, 0, mag).astype(F))).astype(F)
    m = ((s - F(0.5)).astype(F) * F(voxel)).astype(F)
    return np.where(q < 0, -m, m).astype(F)


def distance_map(tsdf, weight, voxel, max_distance=2.0, min_weight=1, flags=0, unbounded=separable):
    """The whole rule over (dz, dy, dx) planes: dict(sq int32, cls uint8, dist float32, counts (4,) int64, R)."""
    R = radius(max_distance, voxel)
    assert 1 <= R <= 1024, R
    cls = classes(tsdf, weight, min_weight)
    sq = signed_sq(unbounded(obstacles(cls, flags)), R)
    counts = np.array([(cls == 0).sum(), (cls == 1).sum(), (cls == 2).sum(), (np.abs(sq.astype(np.int64)) == FAR).sum()], np.int64)
    return dict(sq=sq, cls=cls, dist=metric(sq, R, voxel), counts=counts, R=R)


def query(sq, cls, dims, voxel, origin, R, points):
    """THE QUERY RULE for the world points (3, n): dict(dist (n,), grad (3, n), status (n,) uint8)."""
    pts = np.asarray(points, F)

    class View:  # the volume as tsdf_raycast_model.cell reads it
        pass
    View.dims, View.voxel, View.origin = tuple(dims), F(voxel), np.asarray(origin, F)
    n = pts.shape[1]
    if min(dims) < 2:  # (a dim of 1: no cell at all, every point is out of range)
        return dict(dist=np.zeros(n, F), grad=np.zeros((3, n), F), status=np.full(n, Q_OUTSIDE, np.uint8))
    with np.errstate(all="ignore"):
        inr, i, w = rm.cell(View, [pts[0], pts[1], pts[2]])
        e = rm.corners(metric(np.asarray(sq), R, voxel), i)  # (cell 0 where out of range: the gathers stay in bounds)
        q8 = np.array(rm.corners(np.asarray(sq), i)).reshape(8, n)
        c8 = np.array(rm.corners(np.asarray(cls), i)).reshape(8, n)
        dist = rm.trilerp(e, w).astype(F)
        g = [(ga / F(voxel)).astype(F) for ga in sdf_track_model.gradient(e, w)]
    status = ((np.abs(q8.astype(np.int64)) == FAR).any(0) * Q_FAR + (c8 == UNKNOWN).any(0) * Q_UNKNOWN).astype(np.uint8)
    dist = np.where(inr, dist, F(0)).astype(F)
    grad = np.stack([np.where(inr, ga, F(0)).astype(F) for ga in g])
    return dict(dist=dist, grad=grad, status=np.where(inr, status, Q_OUTSIDE).astype(np.uint8))
