"""The pyramid family (K24) as a thread script, in the style of tests/thread_cases.py: one function that makes every call
of the family on a context it is handed and returns its outputs as a list of (label, bytes).  tests/
test_gpu_pyramid_threads.py runs it alone on fresh contexts, then on eight threads at once, each thread on contexts of
its own, and compares byte for byte.

The calls: build_pyramid with and without smoothing, at 2, 3 and 8 levels (one launch with the second stage off, one
launch of both, chained launches with an odd last level) and two cutoffs; pyramid_shape and pyramid_level of every
level; backproject_level as the source, and as the target with normals; a build of another shape on the same context;
a level the pyramid does not have."""
import numpy as np

import bilateral_model as bm
import pyramid_model as pm
from icp_slam_prototype_amd import binding, depth

CASES = (("68x260", 8, None), ("room_37x53", 2, None), ("room_120x160", 3, dict(radius=2, sigma_range=20.0)),
         ("room_masked", 3, None), ("cutoff_1", 4, None))
P5 = np.full(3, 5, np.float32)


def script(ctx):
    """Every call of the family, on `ctx`.  Returns [(label, bytes)]."""
    out = []
    fx, cx = bm.intrinsics(120)
    for name, levels, smooth in CASES:
        img, K = pm.case(name)
        p = depth.pyramid_params(levels=levels, range_cutoff=K)
        b = None if smooth is None else depth.bilateral_params(**smooth)
        shapes = depth.build_pyramid(ctx, img, p, smooth=b)
        out.append((f"{name}.shapes", np.int32(shapes).tobytes()))
        for l in range(levels):
            assert depth.pyramid_shape(ctx, l) == shapes[l]
            out.append((f"{name}.level{l}", depth.pyramid_level(ctx, l).tobytes()))
        try:
            depth.pyramid_level(ctx, levels)
            rc = binding.OK
        except binding.IcpkError as e:
            rc = e.code
        out.append((f"{name}.beyond", np.int32(rc).tobytes()))
        last = levels - 1
        n = depth.backproject_level(ctx, last, which=0, fx=fx, cx=cx, offset=P5)
        out.append((f"{name}.source", np.int32(n).tobytes() + ctx.get_source().tobytes()))
        n = depth.backproject_level(ctx, min(1, last), which=1, normals_mode=binding.NORMALS_CROSS, fx=fx, cx=cx)
        out.append((f"{name}.target", np.int32(n).tobytes() + ctx.get_target().tobytes() + ctx.get_target_normals().tobytes()))
    return out


def model_levels():
    """{label: bytes} of the levels the script downloads, from tests/pyramid_model.py"""
    want = {}
    for name, levels, smooth in CASES:
        img, K = pm.case(name)
        if smooth is not None:
            img = depth.bilateral_host(img, depth.bilateral_params(**smooth))
        for l, a in enumerate(pm.pyramid(img, levels, K)):
            want[f"{name}.level{l}"] = a.tobytes()
    return want


def first_difference(a, b):
    """None, or (label, byte offset) of the first output in which two runs of the script differ"""
    if [k for k, _ in a] != [k for k, _ in b]:
        return "the labels", 0
    for (k, x), (_, y) in zip(a, b):
        if x != y:
            n = min(len(x), len(y))
            return k, next((i for i in range(n) if x[i] != y[i]), n)
    return None
