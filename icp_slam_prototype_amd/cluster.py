"""DBSCAN clustering of one of a context's clouds (K33): which points belong together.  dbscan() labels the working
source or the target on the device by THE CLUSTER RULE of include/icpk.h and, unless labels_only, keeps the points of
the selected clusters; clusters() brings the record to the host; dbscan_host() is the rule as the library's literal
O(n^2) host program, with no context.  Everything runs through one binding.Context.  Nothing of the rule is computed here;
the record's n_noise, n_out and n_dropped are counted on the host from the arrays the library returned (the ABI returns
the first two from icpk_cluster_dbscan only, and n_dropped not at all: the dropped points are those with count 0)."""
import ctypes as C

import numpy as np

from . import binding


def _params(eps, min_points, min_size, max_size, largest_only):
    return binding.ClusterParams(float(eps), int(min_points), int(min_size), int(max_size), 1 if largest_only else 0)


def dbscan(ctx, which, eps, min_points, min_size=1, max_size=0, largest_only=False, labels_only=False):
    """icpk_cluster_dbscan on the working source (which = 0) or the target (1): a point with at least min_points
    neighbours within eps (itself included) is a core point, clusters are the connected components of the core points,
    a border point joins its nearest core neighbour's cluster, everything else is noise.  Kept: the points of clusters
    with min_size <= size <= max_size (0: no upper bound), with largest_only of the largest cluster alone.  labels_only:
    the cloud stays as it is, only clusters() changes.  Returns (n_clusters, n_noise, n_out)."""
    p = _params(eps, min_points, min_size, max_size, largest_only)
    nc, nn, no = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    ctx._chk(ctx._lib.icpk_cluster_dbscan(ctx._h, int(which), C.byref(p), binding.CLUSTER_LABELS_ONLY if labels_only else 0,
                                          C.byref(nc), C.byref(nn), C.byref(no)))
    return nc.value, nn.value, no.value


def _record(n, nc, call):
    """the arrays of a record of n points and nc clusters, filled by call(labels, core, count, nearest, out_index,
    sizes, first) -- each at exactly its size but for the one spare entry an empty array needs"""
    ip, u8 = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    per_point = [np.zeros(max(n, 1), np.int32) for _ in range(4)]
    core = np.zeros(max(n, 1), np.uint8)
    sizes, first = np.zeros(max(nc, 1), np.int32), np.zeros(max(nc, 1), np.int32)
    labels, count, nearest, oidx = per_point
    call(labels.ctypes.data_as(ip), core.ctypes.data_as(u8), count.ctypes.data_as(ip), nearest.ctypes.data_as(ip),
         oidx.ctypes.data_as(ip), sizes.ctypes.data_as(ip), first.ctypes.data_as(ip))
    count = count[:n]
    return dict(n_in=n, n_clusters=nc, labels=labels[:n], core=core[:n], count=count, nearest_core=nearest[:n],
                out_index=oidx[:n], sizes=sizes[:nc], first=first[:nc], n_noise=int((labels[:n] < 0).sum()),
                n_out=int((oidx[:n] >= 0).sum()), n_dropped=int((count == 0).sum()))


def clusters(ctx):
    """icpk_get_clusters, the record of the last dbscan(): dict(n_in, n_clusters, labels (n_in,) int32: -1 for noise,
    core (n_in,) uint8, count (n_in,) int32: neighbours within eps, nearest_core (n_in,) int32: itself for a core point,
    the partner of a border point, -1 for noise, out_index (n_in,) int32: the position in the selected cloud or -1,
    sizes and first (n_clusters,) int32: members and representative of every cluster, n_noise, n_out, and n_dropped: the
    non-finite points, which are the points with count 0)."""
    n, nc = C.c_int32(0), C.c_int32(0)
    ctx._chk(ctx._lib.icpk_get_clusters(ctx._h, C.byref(n), C.byref(nc), None, None, None, None, None, None, None))
    return _record(n.value, nc.value, lambda *a: ctx._chk(ctx._lib.icpk_get_clusters(ctx._h, None, None, *a)))


def dbscan_host(points, eps, min_points, min_size=1, max_size=0, largest_only=False):
    """icpk_cluster_host (host only, O(n^2)): the record of clusters() for points (3, n) float32, plus `points`: the
    selected cloud."""
    pts = np.ascontiguousarray(points, np.float32).reshape(3, -1)
    n = pts.shape[1]
    p = _params(eps, min_points, min_size, max_size, largest_only)
    lib = binding.load()
    nc = C.c_int32(0)

    def chk(rc):
        if rc != binding.OK:
            raise binding.IcpkError(rc, "icpk_cluster_host")

    chk(lib.icpk_cluster_host(binding._fp(pts), n, C.byref(p), C.byref(nc), None, None, None, None, None, None, None, None, None))
    out = _record(n, nc.value, lambda *a: chk(lib.icpk_cluster_host(binding._fp(pts), n, C.byref(p), None, None, None, *a)))
    out["points"] = pts[:, out["out_index"] >= 0]
    return out
