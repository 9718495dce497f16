"""Smoothing a depth frame before its vertex and normal maps are made (K22): the exact bilateral filter of
include/icpk.h, THE BILATERAL RULE.  Holes stay holes, noise is averaged, and a depth step of K units or more is never
averaged across; everything is integer, so the device, the host function and a model in numpy give the same bytes.

    smooth = bilateral_depth_image(ctx, depth)                       # (rows, cols) uint16, the validity mask kept
    n = backproject_smoothed(ctx, depth, which=1, normals_mode=binding.NORMALS_CROSS)   # ... or straight to the cloud
    tracker = tsdf.ModelTracker(vol, bilateral=True)                 # smoothed frames are tracked, raw frames fused

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
