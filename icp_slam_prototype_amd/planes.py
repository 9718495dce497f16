"""RANSAC plane segmentation of one of a context's clouds (K34): which points are the floor, the wall, the table top.
segment() labels the working source or the target on the device by THE PLANE RULE of include/icpk.h and, unless
labels_only, keeps what is left when the planes are taken out (or, with keep_inliers, the points of the planes); planes()
brings the record to the host; segment_host() is the rule as the library's literal O(P H n) host program, with no context;
fit_host() is the refit alone.  Everything runs through one binding.Context.  Nothing of the rule is computed here."""
import ctypes as C

import numpy as np

from . import binding


def _params(distance_threshold, n_hypotheses, max_planes, min_inliers, seed, select_plane):
    return binding.PlaneParams(int(seed), float(distance_threshold), int(n_hypotheses), int(max_planes), int(min_inliers),
                               int(select_plane), 0)


def _flags(labels_only, keep_inliers):
    return (binding.PLANE_LABELS_ONLY if labels_only else 0) | (binding.PLANE_KEEP_INLIERS if keep_inliers else 0)


def default_params():
    """icpk_default_plane_params"""
    p = binding.PlaneParams()
    binding.load().icpk_default_plane_params(C.byref(p))
    return p


def segment(ctx, which, distance_threshold=0.01, n_hypotheses=256, max_planes=4, min_inliers=1000, seed=0, labels_only=False,
            keep_inliers=False, select_plane=-1):
    """icpk_segment_planes on the working source (which = 0) or the target (1): up to max_planes rounds of a seeded RANSAC
    of n_hypotheses planes each over the points not yet on a plane, the winner refitted to its inliers; a plane needs
    min_inliers points within distance_threshold.  Kept: the points on no plane, or with keep_inliers the points of the
    planes (of plane select_plane alone if >= 0).  labels_only: the cloud stays as it is, only planes() changes.  Returns
    (n_planes, n_unassigned, n_out)."""
    p = _params(distance_threshold, n_hypotheses, max_planes, min_inliers, seed, select_plane)
    a, b, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    ctx._chk(ctx._lib.icpk_segment_planes(ctx._h, int(which), C.byref(p), _flags(labels_only, keep_inliers), C.byref(a),
                                          C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def _record(n, n_planes, call):
    """the arrays of a record of n points and n_planes planes, filled by call(labels, out_index, model, info, sums) --
    each at exactly its size but for the one spare entry an empty array needs"""
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    labels, oidx = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    model, sums = np.zeros((max(n_planes, 1), 8)), np.zeros((max(n_planes, 1), 9))
    info = np.zeros((max(n_planes, 1), 6), np.int32)
    call(labels.ctypes.data_as(ip), oidx.ctypes.data_as(ip), model.ctypes.data_as(dp), info.ctypes.data_as(ip),
         sums.ctypes.data_as(dp))
    return dict(n_in=n, n_planes=n_planes, labels=labels[:n], out_index=oidx[:n], model=model[:n_planes], info=info[:n_planes],
                sums=sums[:n_planes], n_out=int((oidx[:n] >= 0).sum()))


def planes(ctx):
    """icpk_get_planes, the record of the last segment(): dict(n_in, n_planes, labels (n_in,) int32: the plane or -1,
    out_index (n_in,) int32: the position in the selected cloud or -1, model (n_planes, 8) float64: normal, d, centre,
    curvature, info (n_planes, 6) int32: the winning hypothesis, its three samples, the RANSAC count, the final count,
    sums (n_planes, 9) float64: the refit's sums, n_out)."""
    n, k = C.c_int32(0), C.c_int32(0)
    ctx._chk(ctx._lib.icpk_get_planes(ctx._h, C.byref(n), C.byref(k), None, None, None, None, None))
    return _record(n.value, k.value, lambda *a: ctx._chk(ctx._lib.icpk_get_planes(ctx._h, None, None, *a)))


def _chk(rc, what):
    if rc != binding.OK:
        raise binding.IcpkError(rc, what)


def segment_host(points, distance_threshold=0.01, n_hypotheses=256, max_planes=4, min_inliers=1000, seed=0, keep_inliers=False,
                 select_plane=-1):
    """icpk_segment_planes_host (host only, O(P H n)): the record of planes() for points (3, n) float32, plus
    n_unassigned and `points`: the selected cloud."""
    pts = np.ascontiguousarray(points, np.float32).reshape(3, -1)
    n = pts.shape[1]
    p = _params(distance_threshold, n_hypotheses, max_planes, min_inliers, seed, select_plane)
    flags = _flags(False, keep_inliers)
    lib = binding.load()
    k, u = C.c_int32(0), C.c_int32(0)
    _chk(lib.icpk_segment_planes_host(binding._fp(pts), n, C.byref(p), flags, C.byref(k), C.byref(u), None, None, None, None,
                                      None, None), "icpk_segment_planes_host")
    out = _record(n, k.value, lambda *a: _chk(lib.icpk_segment_planes_host(binding._fp(pts), n, C.byref(p), flags, None, None,
                                                                            None, *a), "icpk_segment_planes_host"))
    out["n_unassigned"] = u.value
    out["points"] = pts[:, out["out_index"] >= 0]
    return out


def fit_host(sums, count, a, hyp_normal):
    """icpk_plane_fit_host: the refit of THE PLANE RULE alone -> (8,) float64: normal, d, centre, curvature"""
    dp = C.POINTER(C.c_double)
    s = np.ascontiguousarray(sums, np.float64).reshape(9)
    a = np.ascontiguousarray(a, np.float32).reshape(3)
    nrm = np.ascontiguousarray(hyp_normal, np.float64).reshape(3)
    model = np.zeros(8)
    _chk(binding.load().icpk_plane_fit_host(s.ctypes.data_as(dp), int(count), binding._fp(a), nrm.ctypes.data_as(dp),
                                            model.ctypes.data_as(dp)), "icpk_plane_fit_host")
    return model
