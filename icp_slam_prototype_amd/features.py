"""Appearance-based registration of two RGB-D frames with no prior pose (K32): FAST key points, oriented BRIEF
descriptors, Hamming matches, a 3-point RANSAC over the matched 3-D points (K16's icpk_register_global on the match list
the descriptors fill) and, optionally, an ICP refinement of the dense clouds from the pose found.  Everything runs on the
device through one binding.Context; nothing here computes."""
import ctypes as C

import numpy as np

from . import binding


def describe_keypoints(ctx, which, upright=False):
    """icpk_describe_keypoints: the list of the last detect_fast against its image, both on the device, into
    descriptor slot `which` (0 the source side, 1 the target side).  Stream-ordered: no host wait."""
    return ctx._chk(ctx._lib.icpk_describe_keypoints(ctx._h, int(which), binding.BRIEF_UPRIGHT if upright else 0))


def describe_points(ctx, which, img, kp_xy, upright=False):
    """icpk_describe_points: key points (n, 2) float32 (x, y) of any detector against `img` ((rows, cols, 3) BGR or
    (rows, cols) grey uint8) into slot `which`."""
    img, ch = binding._image_arg(img)
    kp = np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
    return ctx._chk(ctx._lib.icpk_describe_points(ctx._h, int(which), img.ctypes.data_as(C.POINTER(C.c_uint8)), img.shape[0],
                                                    img.shape[1], ch, binding._fp(kp), len(kp), binding.BRIEF_UPRIGHT if upright else 0))


def descriptors(ctx, which):
    """icpk_get_descriptors: (kp_xy (n, 2) float32, words (n, 8) uint32, bin (n,) uint8, valid (n,) uint8) of a slot."""
    n = C.c_int32(0)
    ctx._chk(ctx._lib.icpk_get_descriptors(ctx._h, int(which), None, None, None, None, C.byref(n)))
    m = max(n.value, 1)
    kp, words = np.zeros((m, 2), np.float32), np.zeros((m, binding.BRIEF_WORDS), np.uint32)
    b, v = np.zeros(m, np.uint8), np.zeros(m, np.uint8)
    u8 = C.POINTER(C.c_uint8)
    ctx._chk(ctx._lib.icpk_get_descriptors(ctx._h, int(which), binding._fp(kp), words.ctypes.data_as(C.POINTER(C.c_uint32)),
                                             b.ctypes.data_as(u8), v.ctypes.data_as(u8), C.byref(n)))
    return kp[:n.value], words[:n.value], b[:n.value], v[:n.value]


def set_descriptors(ctx, which, kp_xy, words, bin, valid):
    """icpk_set_descriptors: a stored slot back onto the device (kp_xy or bin None: zeros)."""
    words = np.ascontiguousarray(words, np.uint32).reshape(-1, binding.BRIEF_WORDS)
    n = len(words)
    valid = np.ascontiguousarray(valid, np.uint8)
    kp = None if kp_xy is None else np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
    b = None if bin is None else np.ascontiguousarray(bin, np.uint8)
    if len(valid) != n or (kp is not None and len(kp) != n) or (b is not None and len(b) != n):
        raise ValueError("kp_xy, words, bin and valid must have one entry per key point")
    u8 = C.POINTER(C.c_uint8)
    return ctx._chk(ctx._lib.icpk_set_descriptors(ctx._h, int(which), None if kp is None else binding._fp(kp),
                                                    words.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                    None if b is None else b.ctypes.data_as(u8), valid.ctypes.data_as(u8), n))


def described_to_cloud(ctx, which, depth, R=None, t=None, fx=468.60, cx=318.27):
    """icpk_described_to_cloud: detected_to_cloud's rule on the slot's key points; cloud `which` is replaced and the
    map key point -> cloud index stays on the device (descriptor_cloud_map).  Returns the point count."""
    depth = np.ascontiguousarray(depth, np.uint16)
    Rm = binding._f(np.eye(3) if R is None else R).reshape(9)
    tv = binding._f(np.zeros(3) if t is None else t).reshape(3)
    n = C.c_int32(0)
    ctx._chk(ctx._lib.icpk_described_to_cloud(ctx._h, int(which), depth.ctypes.data_as(C.POINTER(C.c_uint16)),
                                                depth.shape[0], depth.shape[1], fx, cx, binding._fp(Rm), binding._fp(tv), C.byref(n)))
    return n.value


def descriptor_cloud_map(ctx, which):
    """icpk_get_descriptor_cloud_map: (n,) int32, every key point's index in cloud `which`, -1 where it was dropped."""
    n = C.c_int32(0)
    ip = C.POINTER(C.c_int32)
    ctx._chk(ctx._lib.icpk_get_descriptor_cloud_map(ctx._h, int(which), None, C.byref(n)))
    m = np.zeros(max(n.value, 1), np.int32)
    ctx._chk(ctx._lib.icpk_get_descriptor_cloud_map(ctx._h, int(which), m.ctypes.data_as(ip), C.byref(n)))
    return m[:n.value]


def match_descriptors(ctx, params=None, **kw):
    """icpk_match_descriptors + icpk_get_descriptor_matches: THE MATCH RULE over the two slots (params a
    BriefMatchParams, or brief_match_params' keywords).  Returns (src_kp, tgt_kp, H, H2) int32, source order; with
    to_clouds the pairs with two cloud points are K16's match list (get_feature_matches, register_global)."""
    p = params if params is not None else binding.brief_match_params(**kw)
    n = C.c_int32(0)
    ctx._chk(ctx._lib.icpk_match_descriptors(ctx._h, C.byref(p), C.byref(n)))
    out = [np.zeros(max(n.value, 1), np.int32) for _ in range(4)]
    ip = C.POINTER(C.c_int32)
    ctx._chk(ctx._lib.icpk_get_descriptor_matches(ctx._h, *[o.ctypes.data_as(ip) for o in out], C.byref(n)))
    return tuple(o[:n.value].copy() for o in out)


def feature_matches(ctx):
    """icpk_get_feature_matches: K16's match list as it stands (src_index, tgt_index int32, D float32)."""
    ip = C.POINTER(C.c_int32)
    m = C.c_int32(0)
    ctx._chk(ctx._lib.icpk_get_feature_matches(ctx._h, None, None, None, C.byref(m)))
    n = max(m.value, 1)
    si, ti, D = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
    ctx._chk(ctx._lib.icpk_get_feature_matches(ctx._h, si.ctypes.data_as(ip), ti.ctypes.data_as(ip), binding._fp(D), C.byref(m)))
    return si[:m.value].copy(), ti[:m.value].copy(), D[:m.value].copy()


class FrameRegistrar:
    """register(bgr_a, depth_a, bgr_b, depth_b) -> the pose that moves frame a's camera coordinates onto frame b's.

    ctx: a binding.Context (its clouds, descriptor slots and match list are overwritten).  fx, cx: the pinhole of both
    images (cx for both axes, as everywhere in this library).  fast_threshold / fast_type: icpk_detect_fast's.  match: a
    BriefMatchParams or None (mutual, H <= max_hamming, no ratio test); ICPK_BRIEF_TO_CLOUDS is always set.
    n_hypotheses, seed, max_dist, edge_similarity: icpk_register_global's.  refine: run icpk_align (Kabsch flavour,
    exactly refine_iterations iterations -- the loop's mean-square threshold would end it at once from a pose this close --
    over the pairs within refine_max_dist) on the two dense clouds from the pose found."""

    def __init__(self, ctx, fx=468.60, cx=318.27, fast_threshold=20, fast_type=binding.FAST_TYPE_7_12, upright=False, match=None,
                 max_hamming=48, n_hypotheses=4096, seed=0, max_dist=0.05, edge_similarity=0.9, refine=True,
                 refine_iterations=30, refine_max_dist=0.05):
        self.ctx, self.fx, self.cx = ctx, float(fx), float(cx)
        self.fast_threshold, self.fast_type, self.upright = int(fast_threshold), fast_type, bool(upright)
        m = match if match is not None else binding.brief_match_params(max_hamming=max_hamming, mutual=True)
        self.match = binding.BriefMatchParams(m.max_hamming, m.ratio_num, m.ratio_den, m.flags | binding.BRIEF_TO_CLOUDS)
        self.global_kw = dict(n_hypotheses=n_hypotheses, seed=seed, max_dist=max_dist, edge_similarity=edge_similarity)
        self.refine, self.refine_iterations, self.refine_max_dist = bool(refine), int(refine_iterations), float(refine_max_dist)

    def describe(self, which, bgr, depth):
        """detect, describe and cloud for one frame into side `which`; returns (key points, cloud points)"""
        c = self.ctx
        c.detect_fast(bgr, threshold=self.fast_threshold, type=self.fast_type, capacity=0)
        describe_keypoints(c, which, upright=self.upright)
        return c.detected_count, described_to_cloud(c, which, depth, fx=self.fx, cx=self.cx)

    def refine_from(self, T, depth_a, depth_b):
        """icpk_align of frame a's dense cloud, moved by T, onto frame b's; returns (the refined pose, stats, status)"""
        c = self.ctx
        T = np.asarray(T, np.float64)
        c.backproject(depth_b, which=1, fx=self.fx, cx=self.cx)
        c.backproject(depth_a, which=0, fx=self.fx, cx=self.cx)
        c.transform_source(T[:3, :3], T[:3, 3])
        c.commit_source()
        Ta, st, rc = c.align(solve=binding.SOLVE_KABSCH, max_iterations=self.refine_iterations, fixed_iterations=1,
                              max_nn_dist=self.refine_max_dist)
        return Ta.astype(np.float64) @ T, st, rc

    def register(self, bgr_a, depth_a, bgr_b, depth_b):
        """Returns dict(T (4, 4) float64: the pose (refined if refine); T_global: the RANSAC's; matches: kept descriptor
        pairs; cloud_matches: those with two 3-D points; inliers: the winning hypothesis' inliers among the key-point
        cloud; keypoints, points: per frame; status: icpk_register_global's (W_TOO_FEW_PAIRS: T is the identity);
        refine_status, refine_stats when refined)."""
        c = self.ctx
        na, pa = self.describe(0, bgr_a, depth_a)
        nb, pb = self.describe(1, bgr_b, depth_b)
        m = match_descriptors(c, self.match)
        g, rc = c.register_global(**self.global_kw)
        out = dict(T=g["T"].astype(np.float64), T_global=g["T"].astype(np.float64), matches=len(m[0]), cloud_matches=g["n_matches"],
                   inliers=g["inliers"], keypoints=(na, nb), points=(pa, pb), status=rc, hypothesis=g["hypothesis"])
        if self.refine and rc == binding.OK:
            out["T"], out["refine_stats"], out["refine_status"] = self.refine_from(out["T_global"], depth_a, depth_b)
        return out
