"""K8 on the device against tests/fast_model.py, bit for bit: count, positions, order and responses of FAST
(icpk_detect_fast), the grey conversion (icpk_bgr_to_gray), and icpk_detected_to_cloud against
icpk_backproject_keypoints + the host pose + icpk_set_source / icpk_set_target."""
import numpy as np
import pytest

import fast_model as fm
from icp_slam_prototype_amd import binding, synth

pytestmark = pytest.mark.gpu

TYPES = (binding.FAST_TYPE_7_12, binding.FAST_TYPE_9_16)


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check(ctx, img, threshold, nonmax, type_):
    kp, resp = ctx.detect_fast(img, threshold=threshold, nonmax=nonmax, type=type_)
    mkp, mresp = fm.detect(img, threshold, nonmax, type_)
    assert len(kp) == len(mkp), (img.shape, threshold, nonmax, type_, len(kp), len(mkp))
    assert same(kp, mkp), (img.shape, threshold, nonmax, type_)
    assert same(resp, mresp), (img.shape, threshold, nonmax, type_)
    return len(kp)


def room_color(rows, cols, k, noise=2.0):
    Rm = synth.rot_xyz_deg(0, 0.4 * k, 0)
    c = np.array([0.01 * k, 0.0, 0.005 * k])
    return (synth.render_room_color(rows, cols, Rm, c, noise_sigma=noise, rng=np.random.default_rng(k)),
            synth.render_room_depth(rows, cols, Rm, c))


def test_random_images_all_settings():
    rng = np.random.default_rng(21)
    with binding.Context(0) as ctx:
        for rows, cols in [(7, 7), (16, 64), (37, 100), (70, 129), (120, 160)]:
            grey = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
            dots = ((rng.random((rows, cols)) < 0.15) * 230).astype(np.uint8)
            bgr = rng.integers(0, 256, (rows, cols, 3)).astype(np.uint8)
            for img in (grey, dots, bgr):
                for type_ in TYPES:
                    for t in (0, 1, 20, 60, 255):
                        for nonmax in (True, False):
                            check(ctx, img, t, nonmax, type_)


@pytest.mark.parametrize("shape", [(480, 640), (424, 512), (250, 333)])
def test_room_frames(shape):
    rows, cols = shape
    with binding.Context(0) as ctx:
        for k in (0, 4):
            bgr, _ = room_color(rows, cols, k)
            for type_ in TYPES:
                for t, nonmax in ((60, True), (20, True), (60, False)):
                    n = check(ctx, bgr, t, nonmax, type_)
                    assert n > 100
            check(ctx, fm.bgr_to_gray(bgr), 60, True, binding.FAST_TYPE_7_12)  # grey input


@pytest.mark.parametrize("case", fm.hand_cases(), ids=lambda c: c[0])
def test_hand_built_cases(case):
    name, img, kw, chk = case
    with binding.Context(0) as ctx:
        kp, resp = ctx.detect_fast(img, threshold=kw["threshold"], nonmax=kw.get("nonmax", True), type=kw["type_"])
        assert chk(kp, resp), (name, kp.tolist(), resp.tolist())


def test_bgr_to_gray_dense_colour_sample():
    with binding.Context(0) as ctx:
        # every (G, R) pair for 16 values of B, plus the full B ramp: 1 M + colours
        for b0 in range(0, 256, 16):
            g, r = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
            b = (b0 + (g + r) % 16) % 256
            bgr = np.stack([b, g, r], -1).astype(np.uint8)
            assert np.array_equal(ctx.bgr_to_gray(bgr), fm.bgr_to_gray(bgr))


def test_capacity_clamp_and_full_count():
    bgr, _ = room_color(240, 320, 2)
    with binding.Context(0) as ctx:
        full, fresp = ctx.detect_fast(bgr)
        n = len(full)
        assert n > 20
        kp, resp = ctx.detect_fast(bgr, capacity=10)
        assert ctx.detected_count == n and same(kp, full[:10]) and same(resp, fresp[:10])
        kp, resp = ctx.detect_fast(bgr, capacity=0)
        assert ctx.detected_count == n and len(kp) == 0
        # NULL outputs: only the count
        img = np.ascontiguousarray(bgr)
        cnt = np.zeros(1, np.int32)
        C = binding.C
        rc = ctx._lib.icpk_detect_fast(ctx._h, img.ctypes.data_as(C.POINTER(C.c_uint8)), 240, 320, 3, 60, 1,
                                       binding.FAST_TYPE_7_12, 5, None, None, cnt.ctypes.data_as(C.POINTER(C.c_int32)))
        assert rc == binding.OK and cnt[0] == n


def test_bad_arguments():
    C = binding.C
    u8, ip = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    img = np.zeros((20, 20, 3), np.uint8)
    p = img.ctypes.data_as(u8)
    cnt = np.zeros(1, np.int32)
    with binding.Context(0) as ctx:
        lib, h = ctx._lib, ctx._h
        q = cnt.ctypes.data_as(ip)
        assert lib.icpk_detect_fast(h, p, 20, 20, 3, 60, 1, binding.FAST_TYPE_5_8, 0, None, None, q) == binding.E_ARG
        assert lib.icpk_detect_fast(h, p, 20, 20, 3, 60, 1, 7, 0, None, None, q) == binding.E_ARG
        assert lib.icpk_detect_fast(h, p, 20, 20, 2, 60, 1, 1, 0, None, None, q) == binding.E_ARG
        assert lib.icpk_detect_fast(h, p, 0, 20, 3, 60, 1, 1, 0, None, None, q) == binding.E_ARG
        assert lib.icpk_detect_fast(h, p, 20, -1, 3, 60, 1, 1, 0, None, None, q) == binding.E_ARG
        assert lib.icpk_detect_fast(h, None, 20, 20, 3, 60, 1, 1, 0, None, None, q) == binding.E_ARG
        d = np.zeros((20, 20), np.uint16)
        eye = np.eye(3, dtype=np.float32)
        z3 = np.zeros(3, np.float32)
        fp = C.POINTER(C.c_float)
        args = (d.ctypes.data_as(C.POINTER(C.c_uint16)), 20, 20, 468.6, 318.27, eye.ctypes.data_as(fp), z3.ctypes.data_as(fp))
        assert lib.icpk_detected_to_cloud(h, *args, 0, q) == binding.E_NOT_SET  # nothing detected yet
        with pytest.raises(ValueError):
            ctx.detect_fast(np.zeros((5, 5, 2), np.uint8))
        kp, _ = ctx.detect_fast(np.zeros((6, 6), np.uint8), threshold=0)
        assert len(kp) == 0 and ctx.detected_count == 0
        assert lib.icpk_detected_to_cloud(h, *args, 2, q) == binding.E_ARG
        assert lib.icpk_detected_to_cloud(h, *args, 0, q) == binding.OK and cnt[0] == 0


def test_detected_to_cloud_matches_host_path(oracle):
    rows, cols = 480, 640
    bgr, depth = room_color(rows, cols, 3)
    rng = np.random.default_rng(4)
    depth = depth.copy()
    depth[rng.random(depth.shape) < 0.3] = 0  # zero-depth key points are dropped
    small = np.ascontiguousarray(depth[:300, :500])  # a depth image smaller than the colour image
    R = synth.rot_xyz_deg(1.0, -2.0, 0.5).astype(np.float32)
    t = np.array([5.0, 5.1, 4.9], np.float32)
    with binding.Context(0) as ctx, binding.Context(0) as ref:
        kp, _ = ctx.detect_fast(bgr)
        assert len(kp) > 100
        for d in (depth, small):
            pts, kept = binding.backproject_keypoints(d, kp)
            assert 0 < pts.shape[1] < len(kp)
            want = oracle.transform_points(pts, R, t)
            for which in (0, 1):
                n = ctx.detected_to_cloud(d, R, t, which=which)
                assert n == pts.shape[1]
                got = ctx.get_source() if which == 0 else ctx.get_target()
                assert same(got, want), which
            # the source it leaves behind aligns exactly as the uploaded one does
            ctx.detected_to_cloud(d, R, t, which=0)
            ctx.detected_to_cloud(d, R, t, which=1)
            ref.set_source(want)
            ref.set_target(want)
            ctx.transform_source(synth.rot_xyz_deg(0, 0.5, 0).astype(np.float32), np.array([0.01, 0, 0], np.float32))
            ref.transform_source(synth.rot_xyz_deg(0, 0.5, 0).astype(np.float32), np.array([0.01, 0, 0], np.float32))
            ctx.commit_source()
            ref.commit_source()
            Ta, sa, ra = ctx.align(max_iterations=5, max_nn_dist=0.1)
            Tb, sb, rb = ref.align(max_iterations=5, max_nn_dist=0.1)
            assert ra == rb and sa.iterations == sb.iterations and same(Ta, Tb)
