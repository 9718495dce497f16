"""K28 without a device: icpk_frame_view_pixels (csrc/frame_view_rule.h, the header the kernel includes) against
tests/frame_view_model.py byte for byte on every case of tests/frame_view_cases.py, the conditions the cases are for,
the condition the loop's tests rest on -- through the pose the view was built at every listed pixel pairs with itself
at distance exactly 0 --, a window of pixels, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import frame_view_cases as fc
import projective_model as jm
from icp_slam_prototype_amd import binding, build


@pytest.fixture(scope="module")
def lib():
    build.build()
    return binding.load()


def host(name, level, **kw):
    c = fc.case(name)
    inten = None if c["intensities"] is None else c["intensities"][level]
    return binding.frame_view_pixels(c["images"][level], c["pose"], fx=c["fx"], cx=c["cx"], level=level, intensity=inten, **kw)


LEVELS = [(name, l) for name in fc.NAMES for l in range(fc.CASES[name]["levels"])]


def test_the_cases_hold_their_condition_before_anything_runs():
    fc.check_conditions()
    assert set(fc.NAMES) >= {"1x1", "3x3", "5x7_hole", "plane", "edge_on", "room", "room_color"}
    assert [fc.case("room")["images"][l].shape for l in fc.ROOM_LEVELS] == [(120, 160), (60, 80), (30, 40)]


def test_through_its_own_pose_a_listed_pixel_pairs_with_itself_at_distance_zero(lib):
    """On the room levels, icpk_projective_pixels at E == P against the model's planes: every listed pixel gets j == i
    and dist exactly 0, every unlisted valid pixel NO_MODEL, every hole NO_DEPTH.  The pose is the room's own (frame
    3's true pose): no pixel of it fails to project onto itself, so the identity was not needed."""
    c = fc.case("room")
    for l in fc.ROOM_LEVELS:
        e = fc.expected("room", l)
        img = c["images"][l]
        fx_l, cx_l = fc.level_camera("room", l)
        p = binding.default_projective_params(level=l, fx=c["fx"], cx=c["cx"])
        pixel, dist, _, pairs = binding.projective_pixels(p, c["pose"], img, e["planes"], img.shape, float(fx_l), float(cx_l), c["pose"])
        want = fc.self_pairs("room", l)
        assert pixel.tobytes() == want["pixel"].tobytes() and dist.tobytes() == want["dist"].tobytes()
        listed, valid = e["listed"].reshape(-1), img.reshape(-1) != 0
        assert pairs == e["n_valid"] == int(listed.sum())
        assert np.array_equal(pixel[listed], np.nonzero(listed)[0]) and not dist.any()
        assert (pixel[valid & ~listed] == jm.NO_MODEL).all() and (pixel[~valid] == jm.NO_DEPTH).all()


@pytest.mark.parametrize("name,level", LEVELS)
def test_host_function_gives_the_models_bytes(lib, name, level):
    want = fc.expected(name, level)
    planes, n_valid, n_no_normal = host(name, level)
    assert (n_valid, n_no_normal) == (want["n_valid"], want["n_no_normal"])
    assert planes.tobytes() == want["planes"].tobytes()
    assert n_valid == int((planes[6] > 0).sum())  # depth > 0 is the validity test


def test_a_window_of_pixels_is_that_part_of_the_image(lib):
    want = fc.expected("room_color", 0)["planes"].reshape(8, -1)
    first, count = 160 * 37 + 11, 1000
    planes, n_valid, _ = host("room_color", 0, first=first, count=count)
    assert planes.tobytes() == np.ascontiguousarray(want[:, first:first + count]).tobytes()
    assert n_valid == int((want[6, first:first + count] > 0).sum())
    planes, n_valid, n_no_normal = host("room", 0, first=5, count=0)
    assert planes.shape == (8, 0) and (n_valid, n_no_normal) == (0, 0)


def test_refusals(lib):
    c = fc.case("3x3")
    img = c["images"][0]

    def code(**kw):
        args = dict(depth=img, pose=c["pose"], fx=c["fx"], cx=c["cx"])
        args.update(kw)
        with pytest.raises(binding.IcpkError) as e:
            binding.frame_view_pixels(**args)
        return e.value.code

    for k in range(16):
        for bad in (np.nan, np.inf):
            P = c["pose"].copy()
            P.reshape(-1)[k] = bad
            assert code(pose=P) == binding.E_ARG
    assert code(pose=None) == binding.E_ARG
    for kw in (dict(fx=0.0), dict(fx=-1.0), dict(fx=np.inf), dict(fx=np.nan), dict(cx=np.nan), dict(cx=np.inf), dict(level=-1),
               dict(level=binding.PYRAMID_MAX_LEVELS), dict(first=-1), dict(first=8, count=2), dict(count=-1)):
        assert code(**kw) == binding.E_ARG, kw
    out = np.zeros(8, np.float32)
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    P = np.ascontiguousarray(c["pose"]).reshape(16)
    u16 = img.ctypes.data_as(C.POINTER(C.c_uint16))
    assert lib.icpk_frame_view_pixels(8.0, 1.0, 0, P.ctypes.data_as(dp), None, None, 3, 3, 0, 1, out.ctypes.data_as(fp), None) == binding.E_ARG
    assert lib.icpk_frame_view_pixels(8.0, 1.0, 0, P.ctypes.data_as(dp), u16, None, 3, 3, 0, 1, None, None) == binding.E_ARG
    assert lib.icpk_frame_view_pixels(8.0, 1.0, 0, P.ctypes.data_as(dp), u16, None, 0, 3, 0, 0, out.ctypes.data_as(fp), None) == binding.E_ARG
    # NULL n_no_normal is allowed; pixel 4 is the one listed
    assert lib.icpk_frame_view_pixels(8.0, 1.0, 0, P.ctypes.data_as(dp), u16, None, 3, 3, 4, 1, out.ctypes.data_as(fp), None) == 1
    assert {"icpk_frame_view_build", "icpk_frame_view_get", "icpk_frame_view_shape", "icpk_frame_view_release",
            "icpk_frame_view_color_gradients", "icpk_projective_set_view", "icpk_frame_view_pixels"} <= set(binding.SYMBOLS)
