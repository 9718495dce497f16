"""Smoothing a depth frame before its vertex and normal maps are made (K22): the exact bilateral filter of
include/icpk.h, THE BILATERAL RULE.  Holes stay holes, noise is averaged, and a depth step of K units or more is never
averaged across; everything is integer, so the device, the host function and a model in numpy give the same bytes.

    smooth = bilateral_depth_image(ctx, depth)                       # (rows, cols) uint16, the validity mask kept
    n = backproject_smoothed(ctx, depth, which=1, normals_mode=binding.NORMALS_CROSS)   # ... or straight to the cloud
    tracker = tsdf.ModelTracker(vol, bilateral=True)                 # smoothed frames are tracked, raw frames fused

A depth pyramid for coarse-to-fine tracking (K24): include/icpk.h, THE PYRAMID RULE.  Level l + 1 is level l at half the
size, every pixel a range-gated 3 x 3 mean centred on pixel (2 r, 2 c) below, so that level l is the frame seen through
(fx / 2^l, cx / 2^l); integers again, the same bytes from the device, the host function and numpy.

    shapes = build_pyramid(ctx, depth, pyramid_params(levels=3), smooth=bilateral_params())   # stays on the device
    half = pyramid_level(ctx, 1)                                     # (rows, cols) uint16 of one level
    n = backproject_level(ctx, 2, which=0, fx=fx, cx=cx)             # fx, cx: the LEVEL-0 intrinsics
    tracker = tsdf.ModelTracker(vol, pyramid=(10, 5, 4))             # 4 iterations at level 2, then 5, then 10 at level 0

The functions take the Context as an argument: the class itself gains no method.
"""
import ctypes as C

import numpy as np

from . import binding

_u16 = C.POINTER(C.c_uint16)


def bilateral_params(**kw):
    """icpk_default_bilateral_params with the given fields replaced: radius, sigma_space, sigma_range, range_cutoff."""
    p = binding.BilateralParams()
    binding.load().icpk_default_bilateral_params(C.byref(p))
    for k, v in kw.items():
        if k not in ("radius", "sigma_space", "sigma_range", "range_cutoff"):
            raise TypeError(f"icpk_bilateral_params has no field {k!r}")
        setattr(p, k, v)
    return p


def _ref(params):
    return None if params is None else C.byref(params)


def _image(depth):
    depth = np.ascontiguousarray(depth, np.uint16)
    if depth.ndim != 2:
        raise ValueError("a (rows, cols) depth image expected")
    return depth


def bilateral_tables(params=None):
    """icpk_bilateral_tables (host only): (ws (2 radius + 1, 2 radius + 1) uint16, wr (K,) uint16)."""
    lib = binding.load()
    K = C.c_int32(0)
    rc = lib.icpk_bilateral_tables(_ref(params), None, None, C.byref(K))
    if rc < 0:
        raise binding.IcpkError(rc, "icpk_bilateral_tables: parameters outside their ranges")
    side = 2 * (3 if params is None else params.radius) + 1
    ws, wr = np.zeros((side, side), np.uint16), np.zeros(K.value, np.uint16)
    lib.icpk_bilateral_tables(_ref(params), ws.ctypes.data_as(_u16), wr.ctypes.data_as(_u16), None)
    return ws, wr


def bilateral_host(depth, params=None):
    """icpk_bilateral_host (host only): the rule over a (rows, cols) uint16 image.  Returns the smoothed image."""
    depth = _image(depth)
    out = np.empty_like(depth)
    rc = binding.load().icpk_bilateral_host(_ref(params), depth.ctypes.data_as(_u16), depth.shape[0], depth.shape[1],
                                            out.ctypes.data_as(_u16))
    if rc < 0:
        raise binding.IcpkError(rc, "icpk_bilateral_host: an empty image or parameters outside their ranges")
    return out


def bilateral_depth_image(ctx, depth, params=None, out=None):
    """icpk_bilateral_depth_image: the rule on the device.  out: the array that receives the result (it may be `depth`
    itself; default: a new one).  Returns it."""
    depth = _image(depth)
    if out is None:
        out = np.empty_like(depth)
    elif out.dtype != np.uint16 or out.shape != depth.shape or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous uint16 array of the image's shape")
    ctx._chk(ctx._lib.icpk_bilateral_depth_image(ctx._h, _ref(params), depth.ctypes.data_as(_u16), out.ctypes.data_as(_u16),
                                                 depth.shape[0], depth.shape[1]))
    return out


def backproject_smoothed(ctx, depth, which=0, normals_mode=None, fx=468.60, cx=318.27, offset=None, params=None):
    """icpk_backproject_smoothed: upload, filter, back-project without the image leaving the device -- Context.backproject
    (normals_mode None) or Context.backproject_with_normals (normals_mode NORMALS_*, which must be 1) on the smoothed
    frame.  Returns the number of points."""
    depth = _image(depth)
    off = None if offset is None else np.ascontiguousarray(offset, np.float32)
    return ctx._chk(ctx._lib.icpk_backproject_smoothed(
        ctx._h, depth.ctypes.data_as(_u16), depth.shape[0], depth.shape[1], fx, cx,
        None if off is None else off.ctypes.data_as(C.POINTER(C.c_float)), int(which),
        -1 if normals_mode is None else int(normals_mode), _ref(params)))


def pyramid_params(**kw):
    """icpk_default_pyramid_params with the given fields replaced: levels, range_cutoff."""
    p = binding.PyramidParams()
    binding.load().icpk_default_pyramid_params(C.byref(p))
    for k, v in kw.items():
        if k not in ("levels", "range_cutoff"):
            raise TypeError(f"icpk_pyramid_params has no field {k!r}")
        setattr(p, k, v)
    return p


def pyramid_shapes(shape, levels):
    """The (rows, cols) of every level of a pyramid over an image of `shape`: level l + 1 halves level l, rounding up."""
    out = [(int(shape[0]), int(shape[1]))]
    for _ in range(1, int(levels)):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def pyramid_host(depth, level, params=None):
    """icpk_depth_pyramid_host (host only): level `level` of the pyramid of a (rows, cols) uint16 image."""
    depth = _image(depth)
    levels = 3 if params is None else params.levels
    if 0 <= int(level) < max(levels, 0) <= binding.PYRAMID_MAX_LEVELS:
        out = np.empty(pyramid_shapes(depth.shape, levels)[int(level)], np.uint16)
    else:
        out = np.empty((1, 1), np.uint16)  # (the call is refused before it writes)
    rc = binding.load().icpk_depth_pyramid_host(_ref(params), depth.ctypes.data_as(_u16), depth.shape[0], depth.shape[1],
                                                int(level), out.ctypes.data_as(_u16))
    if rc < 0:
        raise binding.IcpkError(rc, "icpk_depth_pyramid_host: an empty image, parameters outside their ranges or no such level")
    return out


def build_pyramid(ctx, depth, params=None, smooth=None, intensity=None):
    """icpk_depth_pyramid_build: the pyramid of the frame on the device, resident until the next build.  smooth: a
    bilateral_params object -- level 0 is then the frame after K22; None: the frame as given.  intensity: the frame's
    (rows, cols) float32 image in [0, 1], set beside the pyramid (binding.set_pyramid_intensity; it is never smoothed).
    Returns the list of the levels' (rows, cols)."""
    depth = _image(depth)
    ctx._chk(ctx._lib.icpk_depth_pyramid_build(ctx._h, depth.ctypes.data_as(_u16), depth.shape[0], depth.shape[1],
                                               _ref(params), _ref(smooth)))
    if intensity is not None:
        binding.set_pyramid_intensity(ctx, intensity)
    return pyramid_shapes(depth.shape, 3 if params is None else params.levels)


def pyramid_shape(ctx, level):
    """icpk_depth_pyramid_shape: (rows, cols) of one level of the resident pyramid."""
    r, c = C.c_int32(0), C.c_int32(0)
    ctx._chk(ctx._lib.icpk_depth_pyramid_shape(ctx._h, int(level), C.byref(r), C.byref(c)))
    return r.value, c.value


def pyramid_level(ctx, level):
    """icpk_depth_pyramid_get: one level of the resident pyramid as a (rows, cols) uint16 array."""
    out = np.empty(pyramid_shape(ctx, level), np.uint16)
    ctx._chk(ctx._lib.icpk_depth_pyramid_get(ctx._h, int(level), out.ctypes.data_as(_u16)))
    return out


class Relocaliser:
    """Fern keyframe relocalisation (K27) over one Context: a keyframe database for levels of `shape` (rows, cols) --
    the shape of level params.level of the pyramids the context will hold -- and its parameters (a binding.FernParams,
    or fields of binding.default_fern_params as keywords).

        reloc = Relocaliser(ctx, pyramid_shapes(frame.shape, 3)[2])
        build_pyramid(ctx, frame, pyramid_params(levels=3))
        reloc.process(pose)                 # a tracked frame: encoded, looked up, and harvested when it is new enough
        r = reloc.process(None, k=3)        # a lost frame: r["poses"] are the restarts to try, nearest code first
    """

    def __init__(self, ctx, shape, params=None, **kw):
        self.ctx, self.shape = ctx, (int(shape[0]), int(shape[1]))
        self.params = binding.fern_create(ctx, self.shape[0], self.shape[1], params, **kw)

    @property
    def count(self):
        return binding.fern_count(self.ctx)

    def poses(self, index):
        """the (4, 4) poses of the keyframes `index`"""
        return [binding.fern_keyframe(self.ctx, int(i))[1] for i in index]

    def process(self, pose=None, k=3):
        """binding.fern_process on the resident pyramid, with the poses of the returned keyframes: dict(index, diss,
        valid, added, poses)."""
        r = binding.fern_process(self.ctx, pose, k)
        r["poses"] = self.poses(r["index"])
        return r

    def reset(self):
        binding.fern_reset(self.ctx)

    def save(self, path):
        """the parameters, the level's shape, the codes and the poses as one .npz"""
        kf = [binding.fern_keyframe(self.ctx, i) for i in range(self.count)]
        W = self.params.n_ferns // 8
        np.savez(path, params=np.array([getattr(self.params, f) for f in binding._FERN_FIELDS], np.uint64),
                 shape=np.array(self.shape, np.int64), codes=np.array([c for c, _ in kf], np.uint32).reshape(len(kf), W),
                 poses=np.array([p for _, p in kf], np.float64).reshape(len(kf), 4, 4))

    @classmethod
    def load(cls, ctx, path):
        """a saved database into `ctx` (through binding.fern_add_code, keyframe by keyframe, in order)"""
        with np.load(path) as z:
            fields = {f: int(v) for f, v in zip(binding._FERN_FIELDS, z["params"].astype(np.uint64))}
            self = cls(ctx, tuple(int(v) for v in z["shape"]), **fields)
            for code, pose in zip(z["codes"], z["poses"]):
                binding.fern_add_code(ctx, code, pose)
        return self


def backproject_level(ctx, level, which=0, normals_mode=None, fx=468.60, cx=318.27, offset=None):
    """icpk_depth_pyramid_backproject: Context.backproject (normals_mode None) or Context.backproject_with_normals
    (normals_mode NORMALS_*, which must be 1) of the resident level, read where it lies.  fx, cx: the LEVEL-0 intrinsics;
    the level is seen through (fx / 2^level, cx / 2^level).  Returns the number of points."""
    off = None if offset is None else np.ascontiguousarray(offset, np.float32)
    return ctx._chk(ctx._lib.icpk_depth_pyramid_backproject(
        ctx._h, int(level), fx, cx, None if off is None else off.ctypes.data_as(C.POINTER(C.c_float)), int(which),
        -1 if normals_mode is None else int(normals_mode)))
