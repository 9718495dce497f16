"""THE PYRAMID RULE of include/icpk.h (K24) restated in numpy, the image in int64.  Shared by tests/test_pyramid_host.py,
tests/test_gpu_pyramid.py and tests/pyramid_thread_cases.py, and the cases they run."""
import functools

import numpy as np

import bilateral_model as bm

MAX_LEVELS, DEFAULT_K = 8, 91
LEVEL_COUNTS = [1, 2, 3, 4, 8]  # 4 and 8: chained launches and an odd last level


def shapes(shape, levels):
    out = [(int(shape[0]), int(shape[1]))]
    for _ in range(1, levels):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def level_up(img, K):
    """Level l + 1 of a (rows, cols) uint16 level l."""
    img = np.asarray(img, np.uint16)
    rows, cols = img.shape
    r1, c1 = (rows + 1) // 2, (cols + 1) // 2
    d = np.zeros((rows + 2, cols + 2), np.int64)  # out-of-image positions are 0: skipped like holes
    d[1:1 + rows, 1:1 + cols] = img
    dc = d[1:1 + rows:2, 1:1 + cols:2]
    assert dc.shape == (r1, c1)
    S, D = np.zeros((r1, c1), np.int64), np.zeros((r1, c1), np.int64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            dq = d[1 + dy:1 + dy + 2 * r1 - 1:2, 1 + dx:1 + dx + 2 * c1 - 1:2]
            ok = (dq != 0) & (np.abs(dq - dc) < K)
            w = (2 - abs(dy)) * (2 - abs(dx))
            S += np.where(ok, w, 0)
            D += np.where(ok, w * (dq - dc), 0)
    out = dc + (2 * D + S) // np.maximum(2 * S, 1)  # (// floors towards minus infinity)
    return np.where(dc != 0, out, 0).astype(np.uint16)


def pyramid(img, levels, K=DEFAULT_K):
    """The list of `levels` images, level 0 first."""
    out = [np.array(img, np.uint16)]
    for _ in range(1, levels):
        out.append(level_up(out[-1], K))
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    """(depth (rows, cols) uint16, K) of one named case; callers must not write to the image."""
    rng = np.random.default_rng(24)
    K = DEFAULT_K
    if name == "room_120x160":
        img = bm.room(120, 160)
    elif name == "room_37x53":  # odd sizes: the last row and column have a partly outside window
        img = bm.room(120, 160)[40:77, 60:113].copy()
    elif name in ("1x1", "1x40", "40x1", "2x2", "3x3"):
        r, c = (int(v) for v in name.split("x"))
        img = (5000 + rng.integers(-40, 41, (r, c))).astype(np.uint16)
    elif name == "room_masked":
        img = bm.room(120, 160)
        img = np.where(rng.random(img.shape) < 0.30, img, 0).astype(np.uint16)
    elif name == "all_65535":  # saturation: no gate, and the output is 65535 everywhere
        img, K = np.full((21, 70), 65535, np.uint16), 65536
    elif name == "all_1":
        img = np.full((21, 70), 1, np.uint16)
    elif name == "cutoff_1":  # only equal depths are averaged: plain subsampling
        img, K = bm.room(120, 160)[30:70, 50:120].copy(), 1
    elif name in ("half_planes_odd", "half_planes_even"):  # two constants K apart: neither side may change
        seam = 33 if name.endswith("odd") else 34
        img = np.full((30, 70), 4000, np.uint16)
        img[:, seam:] = 4000 + K
    elif name in ("16x64", "17x65", "65x131", "68x260"):  # one workgroup exactly, one pixel over, several workgroups
        r, c = (int(v) for v in name.split("x"))
        img = bm.room(480, 640)[100:100 + r, 200:200 + c].copy()
        img[rng.random(img.shape) < 0.1] = 0
    elif name == "room_480x640":
        img = bm.room(480, 640)
    else:
        raise KeyError(name)
    img.setflags(write=False)
    return img, K


@functools.lru_cache(maxsize=None)
def expected(name, levels=MAX_LEVELS):
    """The model's pyramid of a case (level l does not depend on how many levels follow it): computed once, read-only."""
    img, K = case(name)
    out = pyramid(img, levels, K)
    for a in out:
        a.setflags(write=False)
    return out


HOST_CASES = ["room_120x160", "room_37x53", "1x1", "1x40", "40x1", "2x2", "3x3", "room_masked", "all_65535", "all_1",
              "cutoff_1", "half_planes_odd", "half_planes_even"]
SUBSAMPLED = ["all_65535", "all_1", "cutoff_1", "half_planes_odd", "half_planes_even"]  # level l + 1 is level l [::2, ::2]
TILE_CASES = ["16x64", "17x65", "65x131", "68x260"]
