"""The reference's mapped nearest-neighbour lookup (icp.cpp:347-486: findMappedNearestNeighborAssociations,
getNearestMappedPoint, processVoxel) restated over the certainty-map model of tests/map_model.py.  Test
infrastructure: the device lookup (K9, icpk_map_nearest) is checked against it.

Two restatements:
  nearest_literal     loops shaped like :371-486, one voxel at a time -- slow, the definition;
  nearest_vectorised  the same result from the map points within 0.75 m of the query: each is placed at the (shell,
                      rank) positions where the walk reads its slot, then the shells are settled in order.  Fast enough
                      for thousands of queries; it falls back to the literal walk when empty voxels can win (query
                      within 0.75 m of the origin).

Both return (d, list, index) with list KEYPOINTS / POINTS, EMPTY (-1: an empty voxel's zero point won, index -1) or
NONE (-2: nothing beat 0.75; d = 0.75, index -1).
"""
import numpy as np

import map_model as mm

H = mm.MAP_HEIGHT
CELLS = H ** 3
MAX_DIST = np.float32(0.75)  # icp.hpp:8 MAX_NN_COLOR_DISTANCE: the starting `shortestDistance`
MIN_DIST = np.float32(0.2)  # MIN_NN_COLOR_DISTANCE: the walk's stop value
MAX_RADIUS = int(np.float32(1.5) / mm.C)  # int(float(MAX_NN_POINT_DISTANCE) / float(CELL_PHYSICAL_HEIGHT)) = 44
EMPTY, NONE = -1, -2
ZERO = (np.float32(0), np.float32(0), np.float32(0))


def pair_dist(q, t):
    """icp.cpp:606-620 with colour weight 0: float differences, double sum of squares, float sqrt (correctly
    rounded).  Vectorised over t (3, n) or a single point."""
    q = np.asarray(q, np.float32)
    t = np.asarray(t, np.float32)
    with np.errstate(all="ignore"):
        if t.ndim == 1:
            d = [np.float64(np.float32(q[k] - t[k])) for k in range(3)]
            return np.sqrt(np.float32(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
        d = [(np.float32(q[k]) - t[k]).astype(np.float64) for k in range(3)]
        return np.sqrt((d[0] * d[0] + d[1] * d[1] + d[2] * d[2]).astype(np.float32))


def voxel_of_flat(f):
    return (f // (H * H), (f // H) % H, f % H)


def slot_point(model, f):
    """What processVoxel (:476-486) reads at flat offset f of pointLookupTable: the point a filled slot names (list
    read as it stands now), or the default content of an empty slot -- the zero point.  (list, index, point)."""
    s = model.slot.get(voxel_of_flat(f))
    if s is not None and s[1] < len(model.lists[s[0]]):
        return s[0], s[1], model.lists[s[0]][s[1]]
    return EMPTY, -1, ZERO


def nearest_literal(model, q):
    """getNearestMappedPoint (:371-473) for one query."""
    q = tuple(np.float32(v) for v in q)
    vx, vy, vz = mm.voxel(q)
    best = [MAX_DIST, NONE, -1]
    d0 = pair_dist(q, ZERO)  # (every empty voxel yields the zero point)

    def process(x, y, z):  # :476-486; the C array indexed [x][y][z] -> flat offset, z unchecked in block 1
        f = (x * H + y) * H + z
        if f < 0 or f >= CELLS:  # outside the table: unpinned, skipped
            return
        lst, idx, p = slot_point(model, f)
        d = d0 if lst == EMPTY else pair_dist(q, p)
        if d < best[0]:
            best[:] = [d, lst, idx]

    process(vx, vy, vz)
    if best[0] < MAX_DIST:
        return tuple(best)
    r = 1
    while best[0] >= MIN_DIST and r < MAX_RADIUS:
        for y in range(vy - r, vy + r):
            for z in range(vz - r, vz + r):
                if vx - r < 0 or vx - r >= H or vx + r < 0 or vx + r >= H or y < 0 or y >= H:
                    continue
                process(vx - r, y, z)
                process(vx + r, y, z)
        for x in range(vx - r + 1, vx + r - 1):
            for z in range(vz - r, vz + r):
                if x < 0 or x >= H or z < 0 or z >= H or vy - r < 0 or vy - r >= H or vy + r < 0 or vy + r >= H:
                    continue
                process(x, vy - r, z)
                process(x, vy + r, z)
        for x in range(vx - r + 1, vx + r - 1):
            for y in range(vy - r + 1, vy + r - 1):
                if x < 0 or x >= H or y < 0 or y >= H or vz - r < 0 or vz - r >= H or vz + r < 0 or vz + r >= H:
                    continue
                process(x, y, vz - r)
                process(x, y, vz + r)
        r += 1
    return tuple(best)


def visits(v, w):
    """The (shell, rank-in-shell) positions at which the walk from voxel v reads the slot of voxel w: the centre
    (0, 0), at most one direct visit at the Chebyshev radius, and at most one block-1 read through a z overrun."""
    vx, vy, vz = v
    X, Y, Z = w
    out = []
    cheb = max(abs(X - vx), abs(Y - vy), abs(Z - vz))
    if cheb == 0:
        return [(0, 0)]

    def block1(x, y, z):
        r = abs(x - vx)
        if r < 1 or r >= MAX_RADIUS or vx - r < 0 or vx + r >= H or not (0 <= y < H):
            return
        if vy - r <= y < vy + r and vz - r <= z < vz + r:
            out.append((r, 2 * ((y - (vy - r)) * 2 * r + (z - (vz - r))) + (1 if x > vx else 0)))

    r = cheb
    if r < MAX_RADIUS:
        b1 = 8 * r * r
        b2 = b1 + 2 * (2 * r - 2) * 2 * r
        if abs(X - vx) == r:
            block1(X, Y, Z)
        elif abs(Y - vy) == r:
            if vy - r >= 0 and vy + r < H and vx - r + 1 <= X < vx + r - 1 and vz - r <= Z < vz + r:
                out.append((r, b1 + 2 * ((X - (vx - r + 1)) * 2 * r + (Z - (vz - r))) + (1 if Y > vy else 0)))
        elif vz - r >= 0 and vz + r < H and vx - r + 1 <= X < vx + r - 1 and vy - r + 1 <= Y < vy + r - 1:
            out.append((r, b2 + 2 * ((X - (vx - r + 1)) * (2 * r - 2) + (Y - (vy - r + 1))) + (1 if Z > vz else 0)))
    # block 1 reads (x, y, z) with z < 0 or z >= 300 at flat (x * 300 + y) * 300 + z: another voxel
    f = (X * H + Y) * H + Z
    for z in (Z - H, Z + H):
        xy, rem = divmod(f - z, H)
        if rem == 0:
            x, y = divmod(xy, H)
            if 0 <= x < H:
                block1(x, y, z)
    return out


class Lookup:
    """The map's filled slots as arrays, for nearest_vectorised."""

    def __init__(self, model):
        vox, pts, tags = [], [], []
        for w, (lst, idx) in model.slot.items():
            if idx < len(model.lists[lst]):
                vox.append(w)
                pts.append(model.lists[lst][idx])
                tags.append((lst, idx))
        self.model = model
        self.vox = np.array(vox, np.int64).reshape(-1, 3)
        self.pts = np.array(pts, np.float32).reshape(-1, 3)
        self.tags = tags
        fin = np.all(np.isfinite(self.pts), axis=1)  # non-finite points never come within 0.75 m of anything
        self.fin = np.flatnonzero(fin)
        self.tree = None
        if len(self.fin):
            try:
                from scipy.spatial import cKDTree
                self.tree = cKDTree(self.pts[self.fin].astype(np.float64))
            except ImportError:
                pass

    def near(self, q):
        """indices of the stored points within 0.75 m of q (a superset of those with pair_dist < 0.75)"""
        if len(self.fin) == 0:
            return np.zeros(0, np.int64)
        if self.tree is not None:
            return self.fin[np.asarray(self.tree.query_ball_point(np.asarray(q, np.float64), 0.7501), np.int64)]
        d = np.abs(self.pts[self.fin] - np.asarray(q, np.float32)).max(axis=1)
        return self.fin[d <= 0.7501]


def visits_many(v, W):
    """visits() for many voxels W (k, 3) at once: arrays (shell, rank, row of W), in no particular order."""
    vx, vy, vz = v
    X, Y, Z = W[:, 0], W[:, 1], W[:, 2]
    rows = np.arange(len(W))
    out = []

    def block1(x, y, z, j):
        r = np.abs(x - vx)
        ok = (r >= 1) & (r < MAX_RADIUS) & (vx - r >= 0) & (vx + r < H) & (y >= 0) & (y < H)
        ok &= (vy - r <= y) & (y < vy + r) & (vz - r <= z) & (z < vz + r)
        rank = 2 * ((y - (vy - r)) * 2 * r + (z - (vz - r))) + (x > vx)
        out.append((r[ok], rank[ok], j[ok]))

    cheb = np.maximum(np.maximum(np.abs(X - vx), np.abs(Y - vy)), np.abs(Z - vz))
    centre = cheb == 0
    out.append((cheb[centre], np.zeros(int(centre.sum()), np.int64), rows[centre]))
    r = cheb
    live = (r > 0) & (r < MAX_RADIUS)
    b1, b2 = 8 * r * r, 8 * r * r + 2 * (2 * r - 2) * 2 * r
    m1 = live & (np.abs(X - vx) == r)
    block1(X[m1], Y[m1], Z[m1], rows[m1])
    m2 = live & ~m1 & (np.abs(Y - vy) == r)
    m2 &= (vy - r >= 0) & (vy + r < H) & (vx - r + 1 <= X) & (X < vx + r - 1) & (vz - r <= Z) & (Z < vz + r)
    rank2 = b1 + 2 * ((X - (vx - r + 1)) * 2 * r + (Z - (vz - r))) + (Y > vy)
    out.append((r[m2], rank2[m2], rows[m2]))
    m3 = live & ~m1 & (np.abs(Y - vy) != r)
    m3 &= (vz - r >= 0) & (vz + r < H) & (vx - r + 1 <= X) & (X < vx + r - 1) & (vy - r + 1 <= Y) & (Y < vy + r - 1)
    rank3 = b2 + 2 * ((X - (vx - r + 1)) * (2 * r - 2) + (Y - (vy - r + 1))) + (Z > vz)
    out.append((r[m3], rank3[m3], rows[m3]))
    f = (X * H + Y) * H + Z
    for z in (Z - H, Z + H):  # block-1 reads through a z overrun
        xy = (f - z) // H
        x, y = xy // H, xy % H
        ok = (x >= 0) & (x < H)
        block1(x[ok], y[ok], z[ok], rows[ok])
    return (np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]),
            np.concatenate([o[2] for o in out]))


def nearest_vectorised(lk, q):
    q = tuple(np.float32(v) for v in q)
    if not all(np.isfinite(q)):
        return (MAX_DIST, NONE, -1)
    if pair_dist(q, ZERO) < MAX_DIST:  # empty voxels can win: the definition
        return nearest_literal(lk.model, q)
    v = mm.voxel(q)
    cand = lk.near(q)
    best = [MAX_DIST, NONE, -1]
    if len(cand) == 0:
        return tuple(best)
    d = pair_dist(q, lk.pts[cand].T)
    keep = d < MAX_DIST
    cand, d = cand[keep], d[keep]
    if len(cand) == 0:
        return tuple(best)
    shell, rank, row = visits_many(v, lk.vox[cand])
    if len(shell) == 0:
        return tuple(best)
    dj = d[row]
    order = np.lexsort((rank, dj.view(np.uint32), shell))  # by shell, then (distance, rank) inside it
    shell, dj, row = shell[order], dj[order], row[order]
    first = np.flatnonzero(np.r_[True, shell[1:] != shell[:-1]])  # each shell's (d, rank) minimum
    for i in first:
        s = shell[i]
        if s > 0 and best[0] < MIN_DIST:
            break
        if dj[i] < best[0]:
            j = cand[row[i]]
            best = [dj[i], lk.tags[j][0], lk.tags[j][1]]
        if s == 0 and best[0] < MAX_DIST:
            break
    return tuple(best)


def nearest_many(model, pts, lk=None):
    """nearest_vectorised over pts (3, n): arrays d (float32), list, index"""
    lk = lk if lk is not None else Lookup(model)
    pts = np.asarray(pts, np.float32)
    n = pts.shape[1]
    d = np.empty(n, np.float32)
    lst = np.empty(n, np.int32)
    idx = np.empty(n, np.int32)
    for i in range(n):
        d[i], lst[i], idx[i] = nearest_vectorised(lk, pts[:, i])
    return d, lst, idx


def voxel_centre(w):
    """a point inside voxel w (by the map's own rule)"""
    p = tuple(np.float32((np.float32(k) + np.float32(0.5)) * mm.C) for k in w)
    assert mm.voxel(p) == tuple(w), (w, p)
    return p


def plant(model, entries):
    """Slots that name points lying elsewhere, built the way a caller can: every voxel w of entries [(w, point)] is
    filled in order through ADD_ASSOCIATED with d = 255 (two hits), then icpk_map_set_points replaces the point list
    with the given points.  Returns (fill points (3, 2n), replacement list (3, n)) for the device."""
    fill = np.array([voxel_centre(w) for w, _ in entries for _ in (0, 1)], np.float32).T.reshape(3, -1)
    pts = np.array([p for _, p in entries], np.float32).T.reshape(3, -1)
    model.update(mm.ADD_ASSOCIATED, fill, 255)
    model.set_points(pts)
    return fill, pts
