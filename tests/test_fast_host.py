"""The FAST contract of include/icpk.h on the CPU: the loop model (FAST_t's structure) and the vectorised model agree,
hand-built images give the known answers, and libicpk.so exports the K8 entry points.  The device is held to the same
model, bit for bit, by tests/test_gpu_fast.py."""
import numpy as np
import pytest

import fast_model as fm
from icp_slam_prototype_amd import binding, build

K8_SYMBOLS = ("icpk_bgr_to_gray", "icpk_detect_fast", "icpk_detected_to_cloud")


@pytest.mark.parametrize("type_", [fm.TYPE_7_12, fm.TYPE_9_16])
def test_loop_and_vectorised_models_agree(type_):
    rng = np.random.default_rng(17 + type_)
    for it in range(10):
        rows, cols = (int(v) for v in rng.integers(6, 40, 2))
        img = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
        if it % 3 == 0:  # sparse bright dots: isolated corners, ties, suppression
            img = ((rng.random((rows, cols)) < 0.2) * 220).astype(np.uint8)
        for t in (0, 1, 20, 60, 255):
            for nonmax in (True, False):
                a = fm.detect_loop(img, t, nonmax, type_)
                b = fm.detect(img, t, nonmax, type_)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (it, t, nonmax)


def test_bgr_input_is_converted_first():
    rng = np.random.default_rng(3)
    bgr = rng.integers(0, 256, (20, 33, 3)).astype(np.uint8)
    g = fm.bgr_to_gray(bgr)
    b, gg, r = (bgr[..., k].astype(np.int64) for k in range(3))
    assert np.array_equal(g, ((1868 * b + 9617 * gg + 4899 * r + 8192) >> 14).astype(np.uint8))
    for f in (fm.detect, fm.detect_loop):
        a, b2 = f(bgr, 20, True, fm.TYPE_9_16), f(g, 20, True, fm.TYPE_9_16)
        assert np.array_equal(a[0], b2[0]) and np.array_equal(a[1], b2[1])


@pytest.mark.parametrize("case", fm.hand_cases(), ids=lambda c: c[0])
def test_hand_built_cases(case):
    name, img, kw, check = case
    for f in (fm.detect_loop, fm.detect):
        kp, resp = f(img, **kw)
        assert check(kp, resp), (name, f.__name__, kp.tolist(), resp.tolist())


def test_ragged_widths_and_tiny_images():
    rng = np.random.default_rng(8)
    for rows, cols in [(6, 6), (7, 7), (7, 40), (40, 7), (9, 65), (17, 63), (18, 129)]:
        img = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
        for type_ in (fm.TYPE_7_12, fm.TYPE_9_16):
            a = fm.detect_loop(img, 10, True, type_)
            b = fm.detect(img, 10, True, type_)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            if rows < 7 or cols < 7:
                assert len(a[0]) == 0


def test_5_8_is_out_of_scope():
    with pytest.raises(ValueError):
        fm.detect(np.zeros((10, 10), np.uint8), 60, True, fm.TYPE_5_8)


def test_library_exports_the_fast_entry_points():
    build.build()
    lib = binding.load()
    for s in K8_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in binding.SYMBOLS
    assert (binding.FAST_TYPE_7_12, binding.FAST_TYPE_9_16) == (fm.TYPE_7_12, fm.TYPE_9_16)
    # no context: ICPK_E_ARG, nothing touched
    n = np.array([-7], np.int32)
    assert lib.icpk_detect_fast(None, None, 10, 10, 1, 60, 1, 1, 0, None, None,
                                n.ctypes.data_as(binding.C.POINTER(binding.C.c_int32))) == binding.E_ARG
