"""K25 without a device: icpk_projective_pixels (csrc/projective_rule.h, the header the kernel includes) against
tests/projective_model.py byte for byte on every case of tests/projective_cases.py -- codes, view pixels, distance bits,
terms -- its terms through the numpy tree against the model's sums, the condition the cases are for, a window of
pixels, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import gicp_model
import projective_cases as pc
import projective_model as jm
from icp_slam_prototype_amd import binding, build


@pytest.fixture(scope="module")
def lib():
    build.build()
    return binding.load()


def params_of(c, **kw):
    return binding.default_projective_params(**dict(dict(level=c["level"], fx=c["fx"], cx=c["cx"], max_dist=c["max_dist"],
                                                         min_normal_cos=c["min_normal_cos"]), **kw))


def host(name, **kw):
    c = pc.case(name)
    v = c["view"]
    return binding.projective_pixels(params_of(c), c["estimate"], c["level_image"], pc.maps_of(name), v["shape"], v["fx"], v["cx"],
                                     c["view_pose"], terms=True, **kw)


def test_the_cases_cover_every_code_and_have_their_pairs():
    pc.check_conditions()
    assert set(pc.NAMES) >= {"room_l0", "room_l1", "plane_behind", "room_yaw30", "holes_frame", "holes_view", "too_far",
                             "normal_gate", "1x1", "7x9", "17x19", "260x260"}
    assert pc.case("260x260")["level_image"].size > 256 * 256 and pc.case("room_l1")["level_image"].shape == (60, 80)


def test_defaults_and_layouts(lib):
    p = binding.default_projective_params()
    assert (p.level, p.max_iterations, p.min_pairs) == (0, 10, 6)
    assert (p.fx, p.cx, p.max_dist, p.min_normal_cos) == (np.float32(468.60), np.float32(318.27), np.float32(0.5), np.float32(-2))
    assert C.sizeof(binding.ProjectiveParams) == 28 and C.sizeof(binding.ProjectiveResult) == 24
    assert C.sizeof(binding.ProjectiveIter) == 12 * 8 + 28 * 8 + 16
    assert (binding.PROJ_NO_DEPTH, binding.PROJ_BEHIND, binding.PROJ_OUTSIDE, binding.PROJ_NO_MODEL, binding.PROJ_TOO_FAR,
            binding.PROJ_NO_NORMAL, binding.PROJ_NORMAL) == jm.CODES


@pytest.mark.parametrize("name", pc.NAMES)
def test_host_function_gives_the_models_bytes(lib, name):
    want = pc.expected(name)
    pixel, dist, terms, pairs = host(name)
    assert pairs == want["count"] == int((pixel >= 0).sum())
    assert pixel.tobytes() == want["pixel"].tobytes()
    assert dist.tobytes() == want["dist"].tobytes()
    assert terms.tobytes() == want["terms"].tobytes()
    # the terms through the canonical tree are the model's sums
    assert gicp_model.canonical(terms).tobytes() == want["sums"].tobytes()
    assert not terms[pixel < 0].any() and not dist[pixel < 0].any()


def test_a_window_of_pixels_is_that_part_of_the_image(lib):
    want = pc.expected("normal_gate")
    first, count = 160 * 37 + 11, 1000
    pixel, dist, terms, pairs = host("normal_gate", first=first, count=count)
    sl = slice(first, first + count)
    assert pixel.tobytes() == want["pixel"][sl].tobytes() and dist.tobytes() == want["dist"][sl].tobytes()
    assert terms.tobytes() == want["terms"][sl].tobytes() and pairs == int((want["pixel"][sl] >= 0).sum())
    assert host("room_l0", first=19200, count=0)[3] == 0


def test_the_loop_model_moves_the_room_frame_towards_its_pose():
    """the model's own loop, which the device's trace is held against: 10 updates run; after 19 (K24's count) the pose is
    within a quarter voxel of the truth, from 83 mm away.  (The first step overshoots in roll -- the weak direction of a
    room seen head on -- and the following ones walk back: 52 mm after 10, 4.3 mm after 19.)"""
    import tsdf_cases as tc

    out = pc.expected_loop("room_l0")
    truth = tc.pose(*tc.ROOM_FOURTH)
    err = lambda T: float(np.linalg.norm((np.linalg.inv(truth) @ T)[:3, 3]))
    assert out["status"] == jm.OK and out["iterations"] == 10 and len(out["trace"]) == 10
    long = pc.expected_loop("room_l0", 19)
    assert err(long["pose"]) < tc.ROOM_VOLUME["voxel"] / 4 < err(pc.case("room_l0")["estimate"])
    assert all(a["sums"].tobytes() == b["sums"].tobytes() for a, b in zip(out["trace"], long["trace"]))
    # the fronto-parallel plane is degenerate at once, and too few pairs stop before any update
    assert jm.align(max_iterations=3, **pc.model_args("plane"))["status"] == jm.W_DEGENERATE
    few = jm.align(max_iterations=3, min_pairs=20000, **pc.model_args("room_l0"))
    assert few["status"] == jm.W_TOO_FEW_PAIRS and few["iterations"] == 0 and len(few["trace"]) == 1


def test_refusals(lib):
    c = pc.case("7x9")
    v = c["view"]
    E = binding.E_ARG

    def code(params=None, pose=None, level=None, view_pose=None, view_fx=None, first=0, count=None):
        try:
            binding.projective_pixels(params_of(c) if params is None else params, c["estimate"] if pose is None else pose,
                                      c["level_image"] if level is None else level, pc.maps_of("7x9"), v["shape"],
                                      v["fx"] if view_fx is None else view_fx, v["cx"], c["view_pose"] if view_pose is None else view_pose,
                                      first=first, count=count)
        except binding.IcpkError as e:
            return e.code
        return 0

    assert code() == 0
    bad = c["estimate"].copy()
    bad[1, 2] = np.nan
    assert code(pose=bad) == E and code(view_pose=bad) == E
    bad[1, 2] = np.inf
    assert code(pose=bad) == E
    for kw in (dict(level=-1), dict(level=8), dict(fx=0.0), dict(fx=-1.0), dict(fx=np.inf), dict(fx=np.nan), dict(cx=np.nan),
               dict(cx=np.inf), dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=np.nan), dict(min_pairs=0),
               dict(max_iterations=0), dict(max_iterations=65), dict(min_normal_cos=np.nan)):
        assert code(params=params_of(c, **kw)) == E, kw
    assert code(params=params_of(c, max_iterations=64, min_pairs=1, max_dist=1e-6)) == 0
    assert code(view_fx=0.0) == E and code(view_fx=np.nan) == E
    assert code(first=-1) == E and code(first=60, count=4) == E and code(count=-1) == E and code(first=63, count=0) == 0
    # NULL pointers
    p = params_of(c)
    assert lib.icpk_projective_pixels(C.byref(p), None, None, 7, 9, None, 120, 160, 1.0, 1.0, None, 0, 1, None, None, None) == E
    lib.icpk_default_projective_params(None)  # (nothing happens)
    assert lib.icpk_projective_associate(None, None, None, None, None) == E
    assert lib.icpk_projective_reduce(None, None, None, None, None) == E
    assert lib.icpk_align_projective(None, None, None, None, None) == E
    assert lib.icpk_get_projective_trace(None, None, 0) == E
