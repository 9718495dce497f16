"""TEST INFRASTRUCTURE: THE CLUSTER RULE of icpk_cluster_dbscan (include/icpk.h, K33) restated in numpy -- the
neighbourhoods from normals_model.neighbour_pairs (a k-d tree's superset filtered by the exact pair distance), the
components of the core points from scipy.sparse.csgraph.connected_components, the border rule by np.minimum.at on the
packed (distance bits, index) keys.  The GPU tests compare the library against it bit for bit.  Never imported by the
package.

brute_force() states the same rule a second time as a literal double loop with a breadth-first search and no spatial
index, for clouds of a few hundred points; test_cluster_host.py holds the two and icpk_cluster_host to one another.
"""
import collections

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

import normals_model as nm

pair_dist = nm.pair_dist
NO_KEY = np.uint64(2 ** 64 - 1)
FIELDS = ("labels", "core", "count", "nearest_core", "out_index", "sizes", "first", "points")


def _select(pts, labels, sizes, min_size, max_size, largest_only, normals):
    """the selection of the rule and what goes with it"""
    n = pts.shape[1]
    size_of = np.where(labels >= 0, sizes[np.maximum(labels, 0)] if sizes.size else 0, 0)
    keep = (labels >= 0) & (size_of >= min_size)
    if max_size != 0:
        keep &= size_of <= max_size
    if largest_only:
        keep &= labels == (int(np.argmax(sizes)) if sizes.size else -1)  # (argmax: the lower label on a tie)
    out_index = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    out = dict(out_index=out_index, keep=keep, n_out=int(keep.sum()), points=pts[:, keep], n_in=n)
    if normals is not None:
        out["normals"] = np.asarray(normals, np.float32).reshape(3, -1)[:, keep]
    return out


def dbscan(pts, eps, min_points, min_size=1, max_size=0, largest_only=False, normals=None):
    """dict(labels, core, count, nearest_core, out_index, sizes, first, n_clusters, n_noise, n_out, n_dropped, keep,
    points[, normals]) of the rule"""
    pts = np.asarray(pts, np.float32).reshape(3, -1)
    n = pts.shape[1]
    assert np.float32(eps) > 0 and min_points >= 1
    i, j = nm.neighbour_pairs(pts, eps)  # every ordered pair with d <= eps, i == j included
    count = np.bincount(i, minlength=n).astype(np.int32)
    core = count >= min_points
    idx = np.arange(n)
    # the components of the core points (every other point is a component of its own here, and never looked at)
    e = core[i] & core[j]
    _, comp = connected_components(coo_matrix((np.ones(int(e.sum()), np.int8), (i[e], j[e])), shape=(n, n)), directed=False) \
        if n else (0, np.zeros(0, np.int64))
    rep = np.full(n + 1, n, np.int64)
    np.minimum.at(rep, comp[core], idx[core])  # the smallest core index of every component
    # a border point's partner: the least (distance bits << 32) | j over its core neighbours
    b = ~core[i] & core[j]
    d = pair_dist(pts[:, i[b]], pts[:, j[b]]).astype(np.float32)
    key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | j[b].astype(np.uint64)
    best = np.full(n, NO_KEY, np.uint64)
    np.minimum.at(best, i[b], key)
    nearest = np.where(core, idx, np.where(best != NO_KEY, (best & np.uint64(0xffffffff)).astype(np.int64), -1))
    root = np.where(nearest >= 0, rep[comp[np.maximum(nearest, 0)]] if n else 0, -1)
    first = np.flatnonzero(core & (root == idx))
    cid = np.full(n + 1, -1, np.int64)
    cid[first] = np.arange(first.size)
    labels = np.where(root >= 0, cid[np.maximum(root, 0)], -1).astype(np.int32)
    sizes = np.bincount(labels[labels >= 0], minlength=first.size).astype(np.int32)
    out = dict(labels=labels, core=core.astype(np.uint8), count=count, nearest_core=nearest.astype(np.int32), sizes=sizes,
               first=first.astype(np.int32), n_clusters=int(first.size), n_noise=int((labels < 0).sum()),
               n_dropped=int((~np.isfinite(pts).all(0)).sum()))
    out.update(_select(pts, labels, sizes, min_size, max_size, largest_only, normals))
    return out


def brute_force(pts, eps, min_points, min_size=1, max_size=0, largest_only=False):
    """The rule once more as a literal double loop and a breadth-first search (small clouds only)."""
    pts = np.asarray(pts, np.float32).reshape(3, -1)
    n = pts.shape[1]
    x, y, z = (pts[c] for c in range(3))
    r = np.float32(eps)
    fin = [bool(np.isfinite(x[i]) and np.isfinite(y[i]) and np.isfinite(z[i])) for i in range(n)]
    near = [[] for _ in range(n)]  # (d, j) of every neighbour, i itself included
    with np.errstate(all="ignore"):
        for i in range(n):
            if not fin[i]:
                continue
            for j in range(n):
                if not fin[j]:
                    continue
                dx, dy, dz = np.float64(x[i] - x[j]), np.float64(y[i] - y[j]), np.float64(z[i] - z[j])
                d = np.sqrt(np.float32((dx * dx + dy * dy) + dz * dz))
                if d <= r:
                    near[i].append((d, j))
    count = [len(v) for v in near]
    core = [count[i] >= min_points for i in range(n)]
    labels = [-1] * n
    nearest = [-1] * n
    first, sizes = [], []
    for s in range(n):  # ascending: the first core point met of a component is its representative
        if not core[s] or labels[s] >= 0:
            continue
        c = len(first)
        first.append(s)
        labels[s] = c
        queue = collections.deque([s])
        while queue:
            u = queue.popleft()
            for _, v in near[u]:
                if core[v] and labels[v] < 0:
                    labels[v] = c
                    queue.append(v)
    for i in range(n):
        if core[i]:
            nearest[i] = i
        elif fin[i]:
            cand = [(d, j) for d, j in near[i] if core[j]]
            if cand:
                nearest[i] = min(cand)[1]
                labels[i] = labels[nearest[i]]
    sizes = [sum(1 for v in labels if v == c) for c in range(len(first))]
    labels, sizes = np.array(labels, np.int32).reshape(n), np.array(sizes, np.int32).reshape(len(first))
    out = dict(labels=labels, core=np.array(core, np.uint8).reshape(n), count=np.array(count, np.int32).reshape(n),
               nearest_core=np.array(nearest, np.int32).reshape(n), sizes=sizes, first=np.array(first, np.int32).reshape(len(first)),
               n_clusters=len(first), n_noise=int((labels < 0).sum()), n_dropped=n - sum(fin))
    out.update(_select(pts, labels, sizes, min_size, max_size, largest_only, None))
    return out


def same(a, b):
    """None if two records agree bit for bit, else the name of the first field that differs"""
    for key in FIELDS:
        u, v = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        if u.shape != v.shape or u.dtype != v.dtype:
            return f"{key} (shape / type: {u.shape} {u.dtype}, {v.shape} {v.dtype})"
        if u.tobytes() != v.tobytes():
            return key
    for key in ("n_clusters", "n_noise", "n_out", "n_dropped"):
        if a[key] != b[key]:
            return key
    return None


def core_partition(rec):
    """the partition of the core points as a set of frozensets of indices"""
    groups = collections.defaultdict(list)
    for i in np.flatnonzero(rec["core"]):
        groups[int(rec["labels"][i])].append(int(i))
    return {frozenset(g) for g in groups.values()}


# ---- the clouds of the tests --------------------------------------------------------------------------------------
def chain(n, eps, order="ascending", seed=5):
    """n points on a line spaced 0.9 eps: one cluster at min_points <= 2, and trees as deep as the order makes them"""
    t = (np.arange(n, dtype=np.float64) * 0.9 * float(np.float32(eps))).astype(np.float32)
    pts = np.stack([t, np.zeros(n, np.float32), np.zeros(n, np.float32)])
    if order == "descending":
        pts = pts[:, ::-1]
    elif order == "shuffled":
        pts = pts[:, np.random.default_rng(seed).permutation(n)]
    return np.ascontiguousarray(pts)


def bridge(tie=False):
    """Two blobs of core points (3 x 3 x 3 lattices of spacing 0.5) whose only link is one non-core point between them:
    at min_points = 8, eps = 1 the blobs' points are core (11 neighbours at a corner) and the bridge (7 with itself, or 3) is
    not.  The bridge
    is nearer to the SECOND blob (higher indices) unless tie: then it is at exactly the same float distance from one
    point of each and must take the lower index.  Returns (points, index of the bridge)."""
    g = np.float32([0.0, 0.5, 1.0])
    blob = np.stack(np.meshgrid(g, g, g, indexing="ij")).reshape(3, -1).astype(np.float32)
    a = blob.copy()
    b = blob.copy()
    b[0] += np.float32(2.75)  # the blobs' faces are 1.75 apart: more than eps
    mid = np.float32([[1.875 if tie else 1.9375], [0.5], [0.5]])  # 0.875 from each face / 0.9375 and 0.8125
    return np.ascontiguousarray(np.concatenate([a, b, mid], axis=1)), 54


def with_clumps(cloud, n_clumps=40, per=12, sigma=0.004, seed=11, gap=0.15):
    """cloud plus n_clumps clumps of `per` points each (normal, sigma) appended: the flying pixels K13 cannot remove.
    Every clump centre is drawn uniformly in the cloud's bounding box with default_rng(seed) and kept when it is more
    than `gap` from the cloud and from the centres before it.  Returns (points, is_stray)."""
    cloud = np.asarray(cloud, np.float32).reshape(3, -1)
    fin = np.isfinite(cloud).all(0)
    tree = cKDTree(cloud[:, fin].astype(np.float64).T)
    lo, hi = cloud[:, fin].min(axis=1).astype(np.float64), cloud[:, fin].max(axis=1).astype(np.float64)
    rng = np.random.default_rng(seed)
    centres = []
    while len(centres) < n_clumps:
        c = rng.uniform(lo, hi)
        if tree.query(c)[0] > gap and all(np.linalg.norm(c - o) > gap for o in centres):
            centres.append(c)
    extra = np.concatenate([c[:, None] + rng.normal(0.0, sigma, (3, per)) for c in centres], axis=1).astype(np.float32)
    stray = np.zeros(cloud.shape[1] + extra.shape[1], bool)
    stray[cloud.shape[1]:] = True
    return np.ascontiguousarray(np.concatenate([cloud, extra], axis=1)), stray


def edge_cases():
    """(name, points, eps, min_points) of the small clouds both the host and the device tests run: each is small enough
    for the host's O(n^2) program."""
    rng = np.random.default_rng(17)
    base = rng.uniform(-0.5, 0.5, (3, 1500)).astype(np.float32)
    dup = base.copy()
    dup[:, 500:750] = dup[:, :250]
    dup[:, 750:800] = dup[:, 0:1]
    nonfin = base.copy()
    nonfin[1, 700] = np.nan
    nonfin[0, 701] = np.inf
    nonfin[2, 702] = -np.inf
    two = np.float32([[0.0, 0.25], [0.0, 0.0], [0.0, 0.0]])  # at distance exactly eps = 0.25
    g = np.float32(0.125) * np.stack(np.meshgrid(np.arange(9), np.arange(9), np.arange(3), indexing="ij")).reshape(3, -1)
    wall = np.ascontiguousarray(g.astype(np.float32))  # neighbours at exactly eps = 0.125: the float `<=` counts them
    out = [("empty", np.zeros((3, 0), np.float32), 0.1, 3),
           ("one, min_points 1", base[:, :1], 0.1, 1), ("one, min_points 2", base[:, :1], 0.1, 2),
           ("two at eps, min_points 2", two, 0.25, 2), ("two at eps, min_points 3", two, 0.25, 3),
           ("two below eps apart", two, float(np.nextafter(np.float32(0.25), np.float32(0))), 2),
           ("identical", np.tile(np.float32([[1.0], [2.0], [3.0]]), (1, 300)), 0.05, 5),
           ("identical, min_points above n", np.tile(np.float32([[1.0], [2.0], [3.0]]), (1, 30)), 0.05, 31),
           ("duplicates", dup, 0.08, 6), ("non-finite", nonfin, 0.08, 4), ("all non-finite", np.full((3, 5), np.nan, np.float32), 0.1, 1),
           ("lattice wall", wall, 0.125, 6), ("lattice wall, every finite point core", wall, 0.125, 1),
           ("random, sparse", base, 0.05, 3), ("random, min_points 1", base, 0.06, 1),
           ("scaled 1e-3", base * np.float32(1e-3), 0.08e-3, 5), ("scaled 1e3", base * np.float32(1e3), 0.08e3, 5)]
    for tie in (False, True):
        pts, _ = bridge(tie)
        out.append((f"bridge tie={tie}", pts, 1.0, 8))
    for order in ("ascending", "descending", "shuffled"):
        out.append((f"chain 2000 {order}", chain(2000, 0.01, order), 0.01, 2))
    return [(name, np.ascontiguousarray(p, np.float32), float(eps), int(mp)) for name, p, eps, mp in out]
