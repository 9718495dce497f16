"""K32 on the device: the descriptors of icpk_describe_points / icpk_describe_keypoints against the numpy model of THE
BRIEF RULE (tests/brief_model.py), byte for byte; the slots' round trip; icpk_described_to_cloud against
icpk_detected_to_cloud; the refusals."""
import ctypes as C

import numpy as np
import pytest

import brief_cases as bc
import brief_model as bm
from icp_slam_prototype_amd import binding
from icp_slam_prototype_amd import features as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with binding.Context(0) as c:
        yield c


def same(got, want):
    return all(np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want))


@pytest.mark.parametrize("shape", bc.IMAGE_SHAPES)
@pytest.mark.parametrize("channels", (1, 3))
def test_describe_points_gives_the_models_bytes(ctx, shape, channels):
    img = bc.random_image(*shape, channels)
    for n in bc.KEYPOINT_COUNTS:  # (workgroup remainders: four key points per workgroup)
        kp = bc.border_keypoints(*shape, n)
        for upright in (False, True):
            F.describe_points(ctx, n % 2, img, kp, upright)
            gkp, w, b, v = F.descriptors(ctx, n % 2)
            assert gkp.tobytes() == kp.tobytes()
            assert same((w, b, v), bm.describe(img, kp, upright)), (shape, channels, n, upright)
    # every pixel and a ring around the image: exactly the pixels B <= x < cols - B, B <= y < rows - B are described
    y, x = np.mgrid[-1:shape[0] + 1, -1:shape[1] + 1]
    kp = np.stack([x.ravel(), y.ravel()], 1).astype(np.float32)
    F.describe_points(ctx, 0, img, kp)
    _, w, b, v = F.descriptors(ctx, 0)
    assert same((w, b, v), bm.describe(img, kp))
    assert int(v.sum()) == max(shape[0] - 30, 0) * max(shape[1] - 30, 0)


def test_describe_points_edges(ctx):
    img = np.full((40, 40), 93, np.uint8)  # constant: m = 0, bin 0, no bit set
    kp = np.float32([[20, 20], [15.5, 16.5], [14.5, 20], [np.nan, 20], [20, np.inf], [-1e30, 3], [24.49, 24.5]])
    F.describe_points(ctx, 1, img, kp)
    _, w, b, v = F.descriptors(ctx, 1)
    assert list(v) == [1, 1, 0, 0, 0, 0, 1] and (b == 0).all() and (w == 0).all()
    rnd = bc.random_image(120, 160, 3)
    kp = bc.border_keypoints(120, 160, 600, seed=3)
    F.describe_points(ctx, 1, rnd, kp)
    _, w, b, v = F.descriptors(ctx, 1)
    assert same((w, b, v), bm.describe(rnd, kp)) and len(set(b.tolist())) == 32
    assert same((w, b, v), binding.brief_describe_host(rnd, kp))
    F.describe_points(ctx, 1, rnd, kp)  # a second call: the same bytes
    assert same(F.descriptors(ctx, 1)[1:], (w, b, v))


def test_describe_keypoints_equals_describe_points_on_the_detected_list():
    bgr, depth = bc.frame(None)
    for img in (bgr, np.ascontiguousarray(bgr[..., 1])):
        with binding.Context(0) as c:
            with pytest.raises(binding.IcpkError) as e:
                F.describe_keypoints(c, 0)
            assert e.value.code == binding.E_NOT_SET
            kp, _ = c.detect_fast(img, threshold=bc.FAST_THRESHOLD)
            assert len(kp) > 500
            for upright in (False, True):
                F.describe_keypoints(c, 0, upright)
                F.describe_points(c, 1, img, kp, upright)
                a, b = F.descriptors(c, 0), F.descriptors(c, 1)
                assert same(a, b) and a[0].tobytes() == kp.tobytes()
                assert same(a[1:], bm.describe(img, kp, upright))
            c.bgr_to_gray(bgr)  # the image of the list is overwritten: nothing to describe against
            with pytest.raises(binding.IcpkError) as e:
                F.describe_keypoints(c, 0)
            assert e.value.code == binding.E_NOT_SET


def test_get_set_round_trip(ctx):
    img = bc.random_image(37, 100, 3)
    kp = bc.border_keypoints(37, 100, 257)
    F.describe_points(ctx, 0, img, kp)
    stored = F.descriptors(ctx, 0)
    F.describe_points(ctx, 0, img, kp[:3], upright=True)  # (the slot holds something else in between)
    F.set_descriptors(ctx, 0, *stored)
    assert same(F.descriptors(ctx, 0), stored)
    F.set_descriptors(ctx, 1, None, stored[1], None, stored[3])
    back = F.descriptors(ctx, 1)
    assert same(back[1::2], stored[1::2]) and not back[0].any() and not back[2].any()
    F.set_descriptors(ctx, 1, np.zeros((0, 2), np.float32), np.zeros((0, 8), np.uint32), np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    assert all(len(a) == 0 for a in F.descriptors(ctx, 1))


@pytest.mark.parametrize("which", (0, 1))
def test_described_to_cloud_is_detected_to_cloud(which):
    bgr, depth = bc.frame("yaw24")
    depth = depth.copy()
    depth[::3, ::5] = 0  # (holes: key points are dropped)
    R = np.float32([[0.8, 0.0, 0.6], [0.0, 1.0, 0.0], [-0.6, 0.0, 0.8]])
    t = np.float32([0.1, -0.2, 0.3])
    with binding.Context(0) as c:
        kp, _ = c.detect_fast(bgr, threshold=bc.FAST_THRESHOLD)
        n = c.detected_to_cloud(depth, R, t, which, fx=bc.FX, cx=bc.CX)
        want = (c.get_source() if which == 0 else c.get_target()).tobytes()
        other = (c.get_target if which == 0 else c.get_source)
        F.describe_keypoints(c, which)
        with pytest.raises(binding.IcpkError) as e:
            F.descriptor_cloud_map(c, which)
        assert e.value.code == binding.E_NOT_SET
        c.set_source(np.zeros((3, 5), np.float32))
        c.set_target(np.ones((3, 7), np.float32))
        held = other().tobytes()
        assert F.described_to_cloud(c, which, depth, R, t, fx=bc.FX, cx=bc.CX) == n
        assert (c.get_source() if which == 0 else c.get_target()).tobytes() == want and other().tobytes() == held
        if which == 0:  # the committed and the working copy, as set_source leaves them
            c.reset_source()
            assert c.get_source().tobytes() == want
        # the map inverts icpk_backproject_keypoints' `kept`
        pts, kept = binding.backproject_keypoints(depth, kp, fx=bc.FX, cx=bc.CX)
        m = F.descriptor_cloud_map(c, which)
        inv = np.full(len(kp), -1, np.int32)
        inv[kept] = np.arange(len(kept))
        assert 0 < len(kept) < len(kp) and n == len(kept) and np.array_equal(m, inv)
        # whatever replaces the cloud drops the map
        (c.set_source if which == 0 else c.set_target)(np.zeros((3, 5), np.float32))
        with pytest.raises(binding.IcpkError) as e:
            F.descriptor_cloud_map(c, which)
        assert e.value.code == binding.E_NOT_SET
        F.described_to_cloud(c, which, depth, R, t, fx=bc.FX, cx=bc.CX)
        F.describe_keypoints(c, which)  # ... and so does filling the slot again
        with pytest.raises(binding.IcpkError) as e:
            F.descriptor_cloud_map(c, which)
        assert e.value.code == binding.E_NOT_SET
        # a slot filled by describe_points clouds in the same way
        F.describe_points(c, which, bgr, kp[:100])
        assert F.described_to_cloud(c, which, depth, R, t, fx=bc.FX, cx=bc.CX) == int((inv[:100] >= 0).sum())
        assert np.array_equal(F.descriptor_cloud_map(c, which), inv[:100])


def test_bad_arguments():
    lib = binding.load()
    img = np.zeros((40, 40), np.uint8)
    kp = np.float32([[20, 20]])
    depth = np.full((40, 40), 5000, np.uint16)
    u8, fp, ip, u16, u32 = (C.POINTER(t) for t in (C.c_uint8, C.c_float, C.c_int32, C.c_uint16, C.c_uint32))
    im, kpp, dp = img.ctypes.data_as(u8), kp.ctypes.data_as(fp), depth.ctypes.data_as(u16)
    R = np.eye(3, dtype=np.float32).ravel()
    t = np.zeros(3, np.float32)
    Rp, tp = R.ctypes.data_as(fp), t.ctypes.data_as(fp)
    n = C.c_int32(7)
    with binding.Context(0) as c:
        h = c._h
        assert lib.icpk_describe_keypoints(None, 0, 0) == binding.E_ARG
        assert lib.icpk_describe_keypoints(h, 0, 0) == binding.E_NOT_SET
        assert lib.icpk_describe_keypoints(h, 2, 0) == binding.E_ARG and lib.icpk_describe_keypoints(h, 0, 2) == binding.E_ARG
        for bad in ((2, im, 40, 40, 1, kpp, 1, 0), (-1, im, 40, 40, 1, kpp, 1, 0), (0, None, 40, 40, 1, kpp, 1, 0),
                    (0, im, 0, 40, 1, kpp, 1, 0), (0, im, 40, 0, 1, kpp, 1, 0), (0, im, 40, 40, 2, kpp, 1, 0),
                    (0, im, 40, 40, 1, None, 1, 0), (0, im, 40, 40, 1, kpp, -1, 0), (0, im, 40, 40, 1, kpp, 1, 2),
                    (0, im, 40, 40, 1, kpp, binding.BRIEF_MAX_KEYPOINTS + 1, 0), (0, im, 1 << 14, 1 << 14, 1, kpp, 1, 0)):
            assert lib.icpk_describe_points(h, *bad) == binding.E_ARG, bad
        for which in (0, 1):  # nothing above filled a slot
            assert lib.icpk_get_descriptors(h, which, None, None, None, None, C.byref(n)) == binding.E_NOT_SET and n.value == 0
            n.value = 7
            assert lib.icpk_described_to_cloud(h, which, dp, 40, 40, 100.0, 20.0, Rp, tp, C.byref(n)) == binding.E_NOT_SET and n.value == 0
            n.value = 7
        assert lib.icpk_match_descriptors(h, None, C.byref(n)) == binding.E_NOT_SET and n.value == 0
        assert lib.icpk_get_descriptor_matches(h, None, None, None, None, C.byref(n)) == binding.E_NOT_SET
        assert lib.icpk_describe_points(h, 0, im, 40, 40, 1, None, 0, 0) == binding.OK  # n = 0 is legal
        assert lib.icpk_get_descriptors(h, 0, None, None, None, None, C.byref(n)) == binding.OK and n.value == 0
        assert lib.icpk_match_descriptors(h, None, None) == binding.E_NOT_SET  # (slot 1 is still empty)
        assert lib.icpk_describe_points(h, 1, im, 40, 40, 1, kpp, 1, 0) == binding.OK
        n.value = 7
        assert lib.icpk_match_descriptors(h, None, C.byref(n)) == binding.OK and n.value == 0
        assert lib.icpk_get_descriptors(h, 2, None, None, None, None, None) == binding.E_ARG
        w = np.zeros((1, 8), np.uint32)
        ok, two, b32 = np.ones(1, np.uint8), np.full(1, 2, np.uint8), np.full(1, 32, np.uint8)
        wp = w.ctypes.data_as(u32)
        assert lib.icpk_set_descriptors(h, 0, None, None, None, ok.ctypes.data_as(u8), 1) == binding.E_ARG
        assert lib.icpk_set_descriptors(h, 0, None, wp, None, None, 1) == binding.E_ARG
        assert lib.icpk_set_descriptors(h, 0, None, wp, None, two.ctypes.data_as(u8), 1) == binding.E_ARG
        assert lib.icpk_set_descriptors(h, 0, None, wp, b32.ctypes.data_as(u8), ok.ctypes.data_as(u8), 1) == binding.E_ARG
        assert lib.icpk_set_descriptors(h, 0, None, wp, None, ok.ctypes.data_as(u8), -1) == binding.E_ARG
        assert lib.icpk_set_descriptors(h, 3, None, wp, None, ok.ctypes.data_as(u8), 1) == binding.E_ARG
        assert lib.icpk_get_descriptors(h, 0, None, None, None, None, C.byref(n)) == binding.OK and n.value == 0  # (refusals left it)
        for bad in ((2, dp, 40, 40, 100.0, 20.0, Rp, tp), (1, None, 40, 40, 100.0, 20.0, Rp, tp), (1, dp, 0, 40, 100.0, 20.0, Rp, tp),
                    (1, dp, 40, 40, 100.0, 20.0, None, tp), (1, dp, 40, 40, 100.0, 20.0, Rp, None)):
            n.value = 7
            assert lib.icpk_described_to_cloud(h, *bad, C.byref(n)) == binding.E_ARG and n.value == 0, bad
        for kw in (dict(max_hamming=-1), dict(max_hamming=257), dict(ratio=(-1, 1)), dict(ratio=(1, 0))):
            p = binding.brief_match_params(**kw)
            assert lib.icpk_match_descriptors(h, C.byref(p), C.byref(n)) == binding.E_ARG
        p = binding.brief_match_params()
        p.flags = 4
        assert lib.icpk_match_descriptors(h, C.byref(p), C.byref(n)) == binding.E_ARG
        p = binding.brief_match_params(to_clouds=True)  # no maps
        assert lib.icpk_match_descriptors(h, C.byref(p), C.byref(n)) == binding.E_NOT_SET
        assert b"icpk_described_to_cloud" in lib.icpk_last_error(h)
