"""icpk_esdf_host and icpk_esdf_query_host (K31, host only: csrc/esdf_rule.h as the kernels include it) against the
numpy models of tests/esdf_model.py, byte for byte; the models against each other and, where scipy imports, against
scipy.ndimage.distance_transform_edt; the refusals and the defaults."""
import ctypes as C

import numpy as np
import pytest

import esdf_cases as ec
import esdf_model as em
from icp_slam_prototype_amd import binding, build


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build()
    return binding.load()


@pytest.mark.parametrize("name", ec.CASES)
def test_host_gives_the_models_bytes(name):
    c, m = ec.case(name), ec.model(name)
    sq, cls, dist, counts = binding.esdf_host(ec.volume_params(name), c["tsdf"], c["weight"], **c["esdf"])
    assert np.array_equal(cls, m["cls"]) and np.array_equal(counts, m["counts"])
    assert np.array_equal(sq, m["sq"])
    assert dist.tobytes() == m["dist"].tobytes()
    assert not (sq == 0).any()  # q is never 0


@pytest.mark.parametrize("name", ec.CASES)
def test_the_two_models_agree(name):
    """the definition itself (O(N^2)) against the three full passes the larger cases are held to"""
    c, m = ec.case(name), ec.model(name)
    in_O = em.obstacles(m["cls"], c["esdf"]["flags"])
    pairs = float(in_O.sum()) * float((~in_O).sum())
    if pairs > em.BRUTE_MAX_PAIRS:
        # the room: too many pairs for the definition as it stands; its boundary voxels alone decide every minimum (a
        # voxel of the other kind with all six neighbours of its own kind has a neighbour that is nearer), so the
        # definition is run over those
        pad = np.pad(in_O, 1, mode="edge")
        same = np.ones(in_O.shape, bool)
        for axis in range(3):
            for s in (0, 2):
                sl = [slice(1, -1)] * 3
                sl[axis] = slice(s, s + in_O.shape[axis])
                same &= pad[tuple(sl)] == in_O
        idx = np.stack(np.nonzero(np.ones(in_O.shape, bool)), 1)
        flat, edge = in_O.reshape(-1), ~same.reshape(-1)
        out = np.empty(flat.size, np.int64)
        out[~flat] = em._nearest_brute(idx[~flat], idx[flat & edge])
        out[flat] = -em._nearest_brute(idx[flat], idx[~flat & edge])
        want = em.signed_sq(out.reshape(in_O.shape), m["R"])
    else:
        want = em.signed_sq(em.brute(in_O), m["R"])
    assert np.array_equal(want, m["sq"])


# the cases with both sets non-empty: distance_transform_edt has no answer where there is no zero
@pytest.mark.parametrize("name", [n for n in ec.CASES if n not in ("one", "empty", "empty_flag", "full")])
def test_scipy_is_a_second_witness(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    c, m = ec.case(name), ec.model(name)
    in_O = em.obstacles(m["cls"], c["esdf"]["flags"])
    assert in_O.any() and not in_O.all()
    # distance_transform_edt: the distance of every non-zero voxel to the nearest zero, in float64; its square rounds
    # back to the integer it came from (< 2^21)
    out_d = np.rint(ndimage.distance_transform_edt(~in_O) ** 2).astype(np.int64)
    in_d = np.rint(ndimage.distance_transform_edt(in_O) ** 2).astype(np.int64)
    assert np.array_equal(em.signed_sq(np.where(in_O, -in_d, out_d), m["R"]), m["sq"])


def test_the_cases_say_what_they_are_for():
    far = em.FAR
    assert (ec.model("empty")["sq"] == far).all() and (ec.model("empty")["cls"] == 0).all()
    assert (ec.model("empty_flag")["sq"] == -far).all()
    assert (ec.model("full")["sq"] == -far).all() and (ec.model("full")["cls"] == 2).all()
    sq = ec.model("corner")["sq"]  # [z, y, x]
    assert sq[0, 0, 5] == 25 and sq[0, 1, 5] == far and sq[0, 4, 3] == 25 and sq[0, 0, 0] == -1
    assert ec.model("one")["sq"].item() == far
    for name in ("odd_r6", "odd_r1", "line_x", "line_y", "room", "room_flag"):  # (line_z: R reaches along the whole line)
        m = ec.model(name)
        mag = np.abs(m["sq"].astype(np.int64))
        assert (m["sq"] > 0).any() and (m["sq"] < 0).any() and (mag == far).any() and (mag < far).any(), name
        assert mag[mag < far].max() <= m["R"] ** 2
    assert ec.model("line_z")["R"] == 699 and (ec.model("sphere")["counts"][3] == 0)
    assert ec.model("odd_r6")["counts"][0] > 100  # unknown voxels, through min_weight 2


def test_sphere_is_within_the_analytic_bound():
    c = ec.case("sphere")
    _, cls, dist, counts = binding.esdf_host(ec.volume_params("sphere"), c["tsdf"], c["weight"], **c["esdf"])
    assert counts[3] == 0 and ec.sphere_bounds_hold(dist, cls)


@pytest.mark.parametrize("name", ec.CASES)
def test_query_host_gives_the_models_bytes(name):
    c, m = ec.case(name), ec.model(name)
    pts = ec.points(name)
    got = binding.esdf_query_host(ec.volume_params(name), m["sq"], m["cls"], pts, **c["esdf"])
    want = em.query(m["sq"], m["cls"], c["dims"], c["voxel"], c["origin"], m["R"], pts)
    assert np.array_equal(got["status"], want["status"])
    assert got["dist"].tobytes() == want["dist"].tobytes() and got["grad"].tobytes() == want["grad"].tobytes()
    assert got["status"][-1] == em.Q_OUTSIDE and got["dist"][-1] == 0  # the NaN
    if min(c["dims"]) >= 2:
        assert (got["status"] != em.Q_OUTSIDE).sum() > 1000
    else:
        assert (got["status"] == em.Q_OUTSIDE).all()
    # n = 0 and n = 1
    assert binding.esdf_query_host(ec.volume_params(name), m["sq"], m["cls"], pts[:, :0], **c["esdf"])["dist"].shape == (0,)
    one = binding.esdf_query_host(ec.volume_params(name), m["sq"], m["cls"], pts[:, 5:6], **c["esdf"])
    assert one["dist"].tobytes() == want["dist"][5:6].tobytes() and one["status"][0] == want["status"][5]


def test_query_status_bits():
    """the room has unknown voxels wherever it has far ones; the corner case is known everywhere and far in places"""
    seen = set()
    for name in ("room", "corner"):
        got = binding.esdf_query_host(ec.volume_params(name), ec.model(name)["sq"], ec.model(name)["cls"], ec.points(name),
                                      **ec.case(name)["esdf"])
        seen |= set(int(s) for s in np.unique(got["status"]))
    assert seen == {0, em.Q_FAR, em.Q_UNKNOWN, em.Q_FAR | em.Q_UNKNOWN, em.Q_OUTSIDE}


def test_defaults():
    p = binding.esdf_params()
    assert (p.min_weight, p.flags) == (1, 0) and p.max_distance == np.float32(2.0)
    assert (binding.ESDF_FAR, binding.ESDF_UNKNOWN_OCCUPIED, binding.ESDF_MAX_RADIUS) == (2 ** 31 - 1, 1, 1024)
    assert C.sizeof(binding.EsdfParams) == 12


@pytest.mark.parametrize("bad", [dict(min_weight=0), dict(min_weight=65536), dict(max_distance=0.0), dict(max_distance=-1.0),
                                 dict(max_distance=float("nan")), dict(max_distance=float("inf")), dict(flags=2),
                                 dict(max_distance=0.06), dict(max_distance=1025 * 0.0625)])
def test_host_refusals(bad):
    """min_weight outside 1 .. 65535, a max_distance that is not finite and > 0, an unknown flag, R = 0 and R = 1025"""
    c = ec.case("corner")
    kw = dict(c["esdf"], **bad)
    with pytest.raises(binding.IcpkError) as e:
        binding.esdf_host(ec.volume_params("corner"), c["tsdf"], c["weight"], **kw)
    assert e.value.code == binding.E_ARG
    with pytest.raises(binding.IcpkError) as e:
        binding.esdf_query_host(ec.volume_params("corner"), ec.model("corner")["sq"], ec.model("corner")["cls"], ec.points("corner"), **kw)
    assert e.value.code == binding.E_ARG


def test_the_radius_is_not_clamped_at_its_ends():
    c = ec.case("corner")
    for R in (1, 1024):
        sq, _, _, _ = binding.esdf_host(ec.volume_params("corner"), c["tsdf"], c["weight"], max_distance=(R + 0.5) * ec.VOXEL)
        assert np.array_equal(sq, em.signed_sq(em.separable(em.obstacles(ec.model("corner")["cls"])), R))


def test_null_arguments_are_refused(lib):
    p, e = ec.volume_params("corner"), binding.esdf_params()
    f = np.zeros(12 ** 3, np.float32)
    w = np.zeros(12 ** 3, np.uint16)
    fp, u16 = C.POINTER(C.c_float), C.POINTER(C.c_uint16)
    assert lib.icpk_esdf_host(None, C.byref(e), f.ctypes.data_as(fp), w.ctypes.data_as(u16), None, None, None, None) == binding.E_ARG
    assert lib.icpk_esdf_host(C.byref(p), C.byref(e), None, w.ctypes.data_as(u16), None, None, None, None) == binding.E_ARG
    assert lib.icpk_esdf_host(C.byref(p), C.byref(e), f.ctypes.data_as(fp), w.ctypes.data_as(u16), None, None, None, None) == binding.OK
    sq, cls = np.ones(12 ** 3, np.int32), np.ones(12 ** 3, np.uint8)
    i32, u8 = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    args = (C.byref(p), C.byref(e), sq.ctypes.data_as(i32), cls.ctypes.data_as(u8))
    none = (None,) * 5
    assert lib.icpk_esdf_query_host(*args, None, None, None, 1, *none) == binding.E_ARG  # NULL coordinates with n > 0
    assert lib.icpk_esdf_query_host(*args, None, None, None, -1, *none) == binding.E_ARG
    assert lib.icpk_esdf_query_host(*args, None, None, None, 0, *none) == binding.OK
    assert lib.icpk_esdf_compute(None, None, None) == binding.E_ARG and lib.icpk_esdf_release(None) == binding.E_ARG
