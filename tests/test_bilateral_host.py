"""K22 on the CPU: the tables and the host function of THE BILATERAL RULE (include/icpk.h) against the numpy model
(tests/bilateral_model.py), the invariants the rule promises, what the filter does to a noisy frame, and every refusal
of the two host functions.  No device work."""
import ctypes as C

import numpy as np
import pytest

import bilateral_model as bm
from icp_slam_prototype_amd import binding, build, depth

U16 = C.POINTER(C.c_uint16)


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build()
    return binding.load()


def run(name):
    """(image, K, the library's output, the model's output from the library's tables) of one case"""
    img, fields = bm.case(name)
    p = depth.bilateral_params(**fields)
    ws, wr = depth.bilateral_tables(p)
    return img, wr.size, depth.bilateral_host(img, p), bm.bilateral(img, ws, wr)


@pytest.mark.parametrize("fields", [dict(), dict(radius=1), dict(radius=6, sigma_space=3.0), dict(sigma_range=12.5),
                                    dict(radius=2, sigma_space=0.7, sigma_range=1365.0), dict(range_cutoff=17),
                                    dict(sigma_range=2000.0, range_cutoff=4096)])
def test_tables(fields):
    p = depth.bilateral_params(**fields)
    ws, wr = depth.bilateral_tables(p)
    f = dict(bm.DEFAULTS, **fields)
    mws, mwr = bm.tables(**f)
    assert ws.shape == mws.shape == (2 * f["radius"] + 1,) * 2 and wr.shape == mwr.shape
    # (the host libm and numpy may round a tie differently)
    assert np.abs(ws.astype(np.int64) - mws).max() <= 1 and np.abs(wr.astype(np.int64) - mwr).max() <= 1
    assert ws[f["radius"], f["radius"]] == 4096 and wr[0] == 4096
    assert np.array_equal(ws, ws.T) and np.array_equal(ws, ws[::-1]) and np.array_equal(ws, ws[:, ::-1])
    assert np.all(np.diff(wr.astype(np.int64)) <= 0)
    K = f["range_cutoff"] or int(np.floor(3 * np.float32(f["sigma_range"]))) + 1
    assert wr.size == K


def test_defaults_are_the_written_ones():
    p = depth.bilateral_params()
    assert (p.radius, p.sigma_space, p.sigma_range, p.range_cutoff) == (3, 2.0, 30.0, 0)
    assert C.sizeof(binding.BilateralParams) == 16
    ws, wr = depth.bilateral_tables(None)  # NULL: the defaults
    assert ws.shape == (7, 7) and wr.size == 91
    img, _ = bm.case("room_37x53")
    assert np.array_equal(depth.bilateral_host(img), depth.bilateral_host(img, p))


@pytest.mark.parametrize("name", bm.HOST_CASES)
def test_host_gives_the_models_bytes(name):
    img, K, got, want = run(name)
    assert got.dtype == np.uint16 and got.tobytes() == want.tobytes()
    # the invariants of the rule
    assert np.array_equal(got != 0, img != 0)
    assert np.abs(got.astype(np.int64) - img.astype(np.int64)).max() <= K - 1
    if name in bm.UNCHANGED:
        assert np.array_equal(got, img)
    elif img.size > 1:
        assert not np.array_equal(got, img)  # (the case exercises the averaging)


def test_in_place_on_the_host(lib):
    img, fields = bm.case("room_masked")
    p = depth.bilateral_params(**fields)
    buf = img.copy()
    assert lib.icpk_bilateral_host(C.byref(p), buf.ctypes.data_as(U16), *img.shape, buf.ctypes.data_as(U16)) == binding.OK
    assert np.array_equal(buf, depth.bilateral_host(img, p))


def test_a_step_of_K_is_never_averaged_across():
    """one unit less than K and the two half-planes do mix: the bound of the rule is tight"""
    img, fields = bm.case("half_planes")
    K = bm.cutoff(fields["sigma_range"])
    near = np.array(img)
    near[:, 33:] -= 1
    out = depth.bilateral_host(near)
    assert not np.array_equal(out, near) and np.array_equal(out[:, :33 - 3], near[:, :33 - 3])
    assert np.array_equal(depth.bilateral_host(img), img) and int(img[0, 33]) - int(img[0, 32]) == K


def test_effect_on_the_noisy_room():
    """The 120 x 160 room with noise_sigma 0.002 and the defaults, against the noiseless render: depth error (RMS, units
    of 0.2 mm) 9.93 -> 4.32, ratio 0.435; median angle of the cross-product normals 2.98 deg -> 0.50 deg, ratio 0.169.
    The bars are the issue's, with room for a different but equivalent normals routine."""
    img, _ = bm.case("room_120x160")
    clean = bm.room(120, 160, noise_sigma=0.0)
    rms0, rms1, ang0, ang1 = bm.effect(img, depth.bilateral_host(img), clean, *bm.intrinsics(120))
    print(f"depth RMS {rms0:.3f} -> {rms1:.3f} (ratio {rms1 / rms0:.3f}); median normal angle {ang0:.3f} -> {ang1:.3f} deg "
          f"(ratio {ang1 / ang0:.3f})")
    assert rms1 <= 0.6 * rms0
    assert ang1 <= 0.35 * ang0


BAD_PARAMS = [dict(radius=0), dict(radius=7), dict(radius=-1), dict(sigma_space=0.0), dict(sigma_space=-1.0),
              dict(sigma_space=float("nan")), dict(sigma_space=float("inf")), dict(sigma_range=0.0),
              dict(sigma_range=-3.0), dict(sigma_range=float("nan")), dict(sigma_range=float("inf")),
              dict(range_cutoff=-1), dict(range_cutoff=4097), dict(sigma_range=1365.4),  # K = 4097: not clamped
              dict(sigma_range=1e30)]


@pytest.mark.parametrize("fields", BAD_PARAMS)
def test_bad_parameters_are_refused(lib, fields):
    p = depth.bilateral_params(**fields)
    ws, wr, K = np.full(169, 7, np.uint16), np.full(4096, 7, np.uint16), C.c_int32(-5)
    assert lib.icpk_bilateral_tables(C.byref(p), ws.ctypes.data_as(U16), wr.ctypes.data_as(U16), C.byref(K)) == binding.E_ARG
    assert K.value == -5 and np.all(ws == 7) and np.all(wr == 7)  # a refused call leaves everything as it was
    img = np.full((4, 5), 900, np.uint16)
    out = np.full((4, 5), 7, np.uint16)
    assert lib.icpk_bilateral_host(C.byref(p), img.ctypes.data_as(U16), 4, 5, out.ctypes.data_as(U16)) == binding.E_ARG
    assert np.all(out == 7)
    with pytest.raises(binding.IcpkError):
        depth.bilateral_host(img, p)
    with pytest.raises(binding.IcpkError):
        depth.bilateral_tables(p)


def test_the_largest_K_is_accepted():
    ws, wr = depth.bilateral_tables(depth.bilateral_params(sigma_range=1365.0))
    assert wr.size == 4096


def test_bad_images_are_refused(lib):
    img = np.full((4, 5), 900, np.uint16)
    out = np.full((4, 5), 7, np.uint16)
    a, o = img.ctypes.data_as(U16), out.ctypes.data_as(U16)
    for args in ((None, a, 4, 5, None), (None, None, 4, 5, o), (None, a, 0, 5, o), (None, a, 4, 0, o), (None, a, -1, 5, o),
                 (None, a, 1 << 14, (1 << 14) + 1, o)):  # NULL images, empty sizes, more than 2^28 pixels
        assert lib.icpk_bilateral_host(*args) == binding.E_ARG
    assert np.all(out == 7)
    with pytest.raises(ValueError):
        depth.bilateral_host(np.zeros(5, np.uint16))
    with pytest.raises(TypeError):
        depth.bilateral_params(sigma=1.0)
