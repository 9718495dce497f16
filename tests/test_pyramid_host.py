"""K24 on the CPU: the host function of THE PYRAMID RULE (include/icpk.h) against the numpy model
(tests/pyramid_model.py), the four consequences the rule promises, the centred-intrinsics check against a direct render,
and every refusal of the host function.  No device work."""
import ctypes as C

import numpy as np
import pytest

import pyramid_model as pm
from icp_slam_prototype_amd import binding, build, depth, synth

U16 = C.POINTER(C.c_uint16)
ROOM_FX, ROOM_CX = 117.15, 79.5  # the 120 x 160 room of tests/tsdf_cases.py


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build()
    return binding.load()


def test_defaults_are_the_written_ones():
    p = depth.pyramid_params()
    assert (p.levels, p.range_cutoff) == (3, 91) and C.sizeof(binding.PyramidParams) == 8
    assert binding.PYRAMID_MAX_LEVELS == pm.MAX_LEVELS == 8
    img, _ = pm.case("room_37x53")
    for l in range(3):
        assert np.array_equal(depth.pyramid_host(img, l), depth.pyramid_host(img, l, p))  # NULL: the defaults
    assert depth.pyramid_shapes((37, 53), 8) == [(37, 53), (19, 27), (10, 14), (5, 7), (3, 4), (2, 2), (1, 1), (1, 1)]


@pytest.mark.parametrize("name", pm.HOST_CASES + pm.TILE_CASES + ["room_480x640"])
def test_host_gives_the_models_bytes(name):
    img, K = pm.case(name)
    want = pm.expected(name)
    p = depth.pyramid_params(levels=pm.MAX_LEVELS, range_cutoff=K)
    got = [depth.pyramid_host(img, l, p) for l in range(pm.MAX_LEVELS)]
    assert [g.shape for g in got] == pm.shapes(img.shape, pm.MAX_LEVELS)
    for l in range(pm.MAX_LEVELS):
        assert got[l].dtype == np.uint16 and got[l].tobytes() == want[l].tobytes(), l
    assert got[0].tobytes() == np.ascontiguousarray(img).tobytes()
    # a level does not depend on how many follow it
    for levels in pm.LEVEL_COUNTS:
        q = depth.pyramid_params(levels=levels, range_cutoff=K)
        assert depth.pyramid_host(img, levels - 1, q).tobytes() == want[levels - 1].tobytes()
    # the consequences of the rule, level by level
    changed = False
    for l in range(1, pm.MAX_LEVELS):
        below, sub, out = got[l - 1], got[l - 1][::2, ::2], got[l]
        assert np.array_equal(out != 0, sub != 0)  # the mask below, subsampled exactly
        assert np.abs(out.astype(np.int64) - sub.astype(np.int64)).max() <= K - 1
        if name in pm.SUBSAMPLED:
            assert np.array_equal(out, sub)
        changed = changed or not np.array_equal(out, sub)
        # never across a step of K or more: the output lies between the counted taps of its window
        lo, hi = window_bounds(below, K)
        m = sub != 0
        assert np.all(out[m] >= lo[m]) and np.all(out[m] <= hi[m])
    if name not in pm.SUBSAMPLED and img.size > 1:
        assert changed  # (the case exercises the averaging)
    if name == "all_65535":
        assert all(np.all(g == 65535) for g in got)
    if name == "room_37x53":
        assert got[-1].shape == (1, 1) and got[-2].shape == (1, 1)


def window_bounds(level, K):
    """per pixel of the level above: the smallest and largest depth among the taps the rule counts"""
    rows, cols = level.shape
    r1, c1 = (rows + 1) // 2, (cols + 1) // 2
    d = np.zeros((rows + 2, cols + 2), np.int64)
    d[1:1 + rows, 1:1 + cols] = level
    dc = d[1:1 + rows:2, 1:1 + cols:2]
    lo, hi = dc.copy(), dc.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            dq = d[1 + dy:1 + dy + 2 * r1 - 1:2, 1 + dx:1 + dx + 2 * c1 - 1:2]
            ok = (dq != 0) & (np.abs(dq - dc) < K)
            lo, hi = np.where(ok, np.minimum(lo, dq), lo), np.where(ok, np.maximum(hi, dq), hi)
    return lo, hi


def test_a_step_of_K_is_never_averaged_across():
    """one unit less than K and the two half-planes do mix: the bound of the rule is tight"""
    for name, seam in (("half_planes_odd", 33), ("half_planes_even", 34)):
        img, K = pm.case(name)
        assert int(img[0, seam]) - int(img[0, seam - 1]) == K
        assert np.array_equal(depth.pyramid_host(img, 1), img[::2, ::2])
        near = np.array(img)
        near[:, seam:] -= 1
        out = depth.pyramid_host(near, 1)
        assert not np.array_equal(out, near[::2, ::2])
        assert np.abs(out.astype(np.int64) - near[::2, ::2].astype(np.int64)).max() <= K - 1


def test_in_place_and_level_0_on_the_host(lib):
    img, K = pm.case("room_masked")
    p = depth.pyramid_params(range_cutoff=K)
    buf = np.array(img)
    assert lib.icpk_depth_pyramid_host(C.byref(p), buf.ctypes.data_as(U16), *img.shape, 1, buf.ctypes.data_as(U16)) == binding.OK
    want = pm.expected("room_masked")[1]
    assert buf.reshape(-1)[:want.size].tobytes() == want.tobytes()
    assert np.array_equal(buf.reshape(-1)[want.size:], np.array(img).reshape(-1)[want.size:])  # exactly the level's size
    assert np.array_equal(depth.pyramid_host(img, 0, p), img)


def test_a_level_is_the_frame_through_the_scaled_intrinsics():
    """The window is symmetric about pixel (2 r, 2 c), so level l of the noiseless 120 x 160 room is the room rendered
    at the level's shape through (fx / 2^l, cx / 2^l): exactly with K = 1, and within 36 (level 1) and 29 (level 2)
    depth units with K = 91 -- the figures of the rule's documentation in include/icpk.h."""
    fx, cx = ROOM_FX, ROOM_CX
    clean = synth.render_room_depth(120, 160, np.eye(3), np.zeros(3), fx, cx)
    direct = {l: synth.render_room_depth(120 >> l, 160 >> l, np.eye(3), np.zeros(3), fx / 2 ** l, cx / 2 ** l) for l in (1, 2)}
    for K, bounds in ((1, {1: 0, 2: 0}), (91, {1: 36, 2: 29})):
        p = depth.pyramid_params(range_cutoff=K)
        for l in (1, 2):
            got = depth.pyramid_host(clean, l, p).astype(np.int64)
            diff = np.abs(got - direct[l].astype(np.int64))
            print(f"K = {K}, level {l}: max {diff.max()}, p99 {np.percentile(diff, 99):.0f}")
            assert np.array_equal(got != 0, direct[l] != 0)
            assert diff.max() <= bounds[l]


def test_effect_on_the_noisy_room():
    """The noisy 120 x 160 room (noise_sigma 0.002, default_rng(7)) against the clean level-1 render: RMS error 10.0
    with plain subsampling (K = 1), 5.28 with K = 91.  The bar: nine independent errors under the weights (1 2 1; 2 4 2;
    1 2 1) / 16 shrink by sqrt(36) / 16 = 0.375; the slant of the surfaces inside a window and the pixels at depth edges,
    where fewer taps count, leave room up to two thirds."""
    fx, cx = ROOM_FX, ROOM_CX
    noisy = synth.render_room_depth(120, 160, np.eye(3), np.zeros(3), fx, cx, 0.002, np.random.default_rng(7))
    clean1 = synth.render_room_depth(60, 80, np.eye(3), np.zeros(3), fx / 2, cx / 2).astype(np.float64)
    rms = {}
    for K in (1, 91):
        got = depth.pyramid_host(noisy, 1, depth.pyramid_params(range_cutoff=K)).astype(np.float64)
        m = (got != 0) & (clean1 != 0)
        rms[K] = float(np.sqrt(np.mean((got[m] - clean1[m]) ** 2)))
    print(f"level-1 RMS against the clean render: K = 1 {rms[1]:.3f}, K = 91 {rms[91]:.3f}")
    assert rms[91] <= (2.0 / 3.0) * rms[1]


BAD_PARAMS = [dict(levels=0), dict(levels=9), dict(levels=-1), dict(range_cutoff=0), dict(range_cutoff=-1),
              dict(range_cutoff=65537)]


@pytest.mark.parametrize("fields", BAD_PARAMS)
def test_bad_parameters_are_refused(lib, fields):
    p = depth.pyramid_params(**fields)
    img = np.full((4, 5), 900, np.uint16)
    out = np.full((4, 5), 7, np.uint16)
    assert lib.icpk_depth_pyramid_host(C.byref(p), img.ctypes.data_as(U16), 4, 5, 0, out.ctypes.data_as(U16)) == binding.E_ARG
    assert np.all(out == 7)  # a refused call leaves everything as it was
    with pytest.raises(binding.IcpkError):
        depth.pyramid_host(img, 0, p)


def test_the_ends_of_the_ranges_are_accepted():
    img = np.full((4, 5), 900, np.uint16)
    for fields in (dict(levels=1), dict(levels=8), dict(range_cutoff=1), dict(range_cutoff=65536)):
        p = depth.pyramid_params(**fields)
        assert depth.pyramid_host(img, p.levels - 1, p).shape == pm.shapes((4, 5), p.levels)[-1]


def test_bad_images_and_levels_are_refused(lib):
    img = np.full((4, 5), 900, np.uint16)
    out = np.full((4, 5), 7, np.uint16)
    a, o = img.ctypes.data_as(U16), out.ctypes.data_as(U16)
    for args in ((None, a, 4, 5, 0, None), (None, None, 4, 5, 0, o), (None, a, 0, 5, 0, o), (None, a, 4, 0, 0, o),
                 (None, a, -1, 5, 0, o), (None, a, 1 << 14, (1 << 14) + 1, 0, o),  # NULL images, empty sizes, > 2^28 pixels
                 (None, a, 4, 5, -1, o), (None, a, 4, 5, 3, o)):                   # a level the pyramid does not have
        assert lib.icpk_depth_pyramid_host(*args) == binding.E_ARG
    assert np.all(out == 7)
    with pytest.raises(ValueError):
        depth.pyramid_host(np.zeros(5, np.uint16), 0)
    with pytest.raises(TypeError):
        depth.pyramid_params(cutoff=1)
    with pytest.raises(binding.IcpkError):
        depth.pyramid_host(img, 3)
