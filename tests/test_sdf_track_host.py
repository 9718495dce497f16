"""K29 without a device: icpk_sdf_pixels (csrc/sdf_track_rule.h, the header the kernel includes) against
tests/sdf_track_model.py byte for byte on every case of tests/sdf_track_cases.py -- codes, cells, distance bits, terms --,
its terms through the numpy tree against the model's sums, the condition the cases are for, a window of pixels, the
refusals, and the analytic check: over the room's exact distance field the normals of accepted pixels agree with the
analytic gradient within a bound derived from the field's second derivatives and the voxel size."""
import ctypes as C

import numpy as np
import pytest

import gicp_model
import sdf_track_cases as sc
import sdf_track_model as sm
import tsdf_cases as tc
import tsdf_model
from icp_slam_prototype_amd import binding, build


@pytest.fixture(scope="module")
def lib():
    build.build()
    return binding.load()


def host(name, **kw):
    c = sc.case(name)
    return binding.sdf_pixels(sc.sdf_params(name, binding), sc.volume_params(name, binding), c["estimate"], c["level_image"],
                              c["vol"].tsdf, c["vol"].weight, terms=True, **kw)


def test_the_cases_cover_every_code_and_have_their_pixels():
    sc.check_conditions()
    assert set(sc.NAMES) >= {"room_l0", "room_l1", "1x1", "7x9", "17x19", "260x260", "outside", "holes", "too_far", "constant",
                             "normal_gate", "plane", "shifted"}
    assert sc.case("room_l0")["level_image"].shape == (120, 160) and sc.case("room_l1")["level_image"].shape == (60, 80)


def test_defaults_and_layouts(lib):
    p = binding.default_sdf_params()
    assert (p.level, p.max_iterations, p.min_weight, p.min_pairs) == (0, 10, 1, 6)
    assert (p.fx, p.cx, p.max_abs_tsdf, p.min_normal_cos) == (np.float32(468.60), np.float32(318.27), np.float32(1.0), np.float32(-2))
    assert C.sizeof(binding.SdfParams) == 8 * 4
    assert (binding.SDF_NO_DEPTH, binding.SDF_OUTSIDE, binding.SDF_UNKNOWN, binding.SDF_TOO_FAR, binding.SDF_NO_GRADIENT,
            binding.SDF_NO_NORMAL, binding.SDF_NORMAL) == sm.CODES
    lib.icpk_default_sdf_params(None)  # (a NULL is ignored)


@pytest.mark.parametrize("name", sc.NAMES)
def test_host_function_gives_the_models_bytes(lib, name):
    want = sc.expected(name)
    cell, value, terms, accepted = host(name)
    assert accepted == want["count"] == int((cell >= 0).sum())
    assert cell.tobytes() == want["cell"].tobytes()
    assert value.tobytes() == want["value"].tobytes()
    assert terms.tobytes() == want["terms"].tobytes()  # tolerance 0, signed zeros included
    assert gicp_model.canonical(terms).tobytes() == want["sums"].tobytes()


def test_a_window_of_pixels_is_that_part_of_the_image(lib):
    want = sc.expected("normal_gate")
    first, count = 160 * 37 + 11, 1000
    cell, value, terms, accepted = host("normal_gate", first=first, count=count)
    assert cell.tobytes() == want["cell"][first:first + count].tobytes()
    assert value.tobytes() == want["value"][first:first + count].tobytes()
    assert terms.tobytes() == want["terms"][first:first + count].tobytes()
    assert accepted == int((want["cell"][first:first + count] >= 0).sum())
    assert host("normal_gate", first=19200, count=0)[3] == 0


def test_the_loop_model_moves_the_room_frame_towards_its_pose():
    """the model's own loop, which the device's trace is held against: all 10 updates run from P3, 83 mm from the truth,
    and every one of the last five estimates is nearer to it than the start"""
    truth = tc.pose(*tc.ROOM_FOURTH)
    out = sc.expected_loop("room_l0")
    assert (out["status"], out["iterations"], len(out["trace"])) == (sm.OK, 10, 10)
    err = [float(np.linalg.norm((np.linalg.inv(truth) @ np.vstack([t["pose"], [0, 0, 0, 1]]))[:3, 3])) for t in out["trace"]]
    err.append(float(np.linalg.norm((np.linalg.inv(truth) @ out["pose"])[:3, 3])))
    print("translation error per iterate, mm:", " ".join(f"{1000 * e:.2f}" for e in err))
    assert max(err[6:]) < err[0]


def test_refusals(lib):
    name = "7x9"
    c = sc.case(name)
    E = binding.E_ARG
    vp = sc.volume_params(name, binding)
    good = lambda **kw: binding.sdf_pixels(sc.sdf_params(name, binding, **kw), vp, c["estimate"], c["level_image"], c["vol"].tsdf,
                                           c["vol"].weight)

    def code_of(call, *a, **kw):
        with pytest.raises(binding.IcpkError) as e:
            call(*a, **kw)
        return e.value.code

    assert good()[3] == sc.expected(name)["count"]
    for kw in (dict(level=-1), dict(level=8), dict(fx=0.0), dict(fx=np.inf), dict(cx=np.nan), dict(min_pairs=0),
               dict(max_iterations=0), dict(max_iterations=65), dict(min_normal_cos=np.nan), dict(max_abs_tsdf=0.0),
               dict(max_abs_tsdf=-0.5), dict(max_abs_tsdf=1.5), dict(max_abs_tsdf=np.nan), dict(min_weight=0),
               dict(min_weight=65536)):
        assert code_of(good, **kw) == E, kw
    assert good(max_abs_tsdf=1.0, min_weight=65535)[3] == 0  # (the ends of both ranges are allowed)
    bad = c["estimate"].copy()
    bad[1, 3] = np.inf
    p = sc.sdf_params(name, binding)
    assert code_of(binding.sdf_pixels, p, vp, bad, c["level_image"], c["vol"].tsdf, c["vol"].weight) == E
    assert code_of(binding.sdf_pixels, p, vp, c["estimate"], c["level_image"], c["vol"].tsdf, c["vol"].weight, first=60, count=4) == E
    assert code_of(binding.sdf_pixels, p, vp, c["estimate"], c["level_image"], c["vol"].tsdf, c["vol"].weight, first=-1, count=1) == E
    for field, value in (("voxel", 0.0), ("trunc", np.nan)):
        v2 = sc.volume_params(name, binding)
        setattr(v2, field, value)
        assert code_of(binding.sdf_pixels, p, v2, c["estimate"], c["level_image"], c["vol"].tsdf, c["vol"].weight) == E
    dp, u16 = C.POINTER(C.c_double), C.POINTER(C.c_uint16)
    P = np.ascontiguousarray(c["estimate"]).reshape(16)
    img = np.ascontiguousarray(c["level_image"])
    cell, value = np.zeros(63, np.int32), np.zeros(63, np.float32)
    f, w = np.ascontiguousarray(c["vol"].tsdf).reshape(-1), np.ascontiguousarray(c["vol"].weight).reshape(-1)
    args = lambda **kw: [kw.get("p", C.byref(p)), kw.get("v", C.byref(vp)), kw.get("P", P.ctypes.data_as(dp)),
                         kw.get("img", img.ctypes.data_as(u16)), 7, 9, kw.get("f", f.ctypes.data_as(C.POINTER(C.c_float))),
                         kw.get("w", w.ctypes.data_as(u16)), 0, 63, kw.get("cell", cell.ctypes.data_as(C.POINTER(C.c_int32))),
                         kw.get("value", value.ctypes.data_as(C.POINTER(C.c_float))), None]
    assert lib.icpk_sdf_pixels(*args()) == sc.expected(name)["count"]
    assert lib.icpk_sdf_pixels(*args(p=None)) >= 0  # (NULL params: the defaults)
    for k in ("v", "P", "img", "f", "w", "cell", "value"):
        assert lib.icpk_sdf_pixels(*args(**{k: None})) == E, k


# ---- the analytic check ---------------------------------------------------------------------------------------------
SPHERE_C, SPHERE_R = np.array([0.35, 0.45, 2.3]), 0.55  # (tsdf_cases.room_distance's sphere)


def room_branches(p):
    """the four signed inner values of tsdf_cases.room_distance at the points (3, n): the field is the least of their
    absolute values; and the gradient of each |.|"""
    p = np.asarray(p, np.float64)
    rel = p - SPHERE_C[:, None]
    rho = np.linalg.norm(rel, axis=0)
    inner = np.array([p[1] - 1.3, p[2] - 3.6, p[0] + 2.1, rho - SPHERE_R])
    unit = np.zeros((4, 3, p.shape[1]))
    unit[0, 1], unit[1, 2], unit[2, 0] = 1.0, 1.0, 1.0
    unit[3] = rel / rho
    return inner, unit * np.sign(inner)[:, None, :], rho


def test_normals_agree_with_the_analytic_gradient_within_what_the_voxel_allows(lib):
    """The planes hold tsdf_cases.room_distance / trunc at the voxel centres, every weight 1.  The room frame is read at
    an estimate 0.23 m off its pose, so that its points lie off the surfaces by varying amounts.

    The bound.  Inside a cell of side h the trilinear interpolant's derivative along x is a convex combination (weights
    from w_y, w_z) of the four difference quotients along the cell's x edges, and each quotient is phi_x at some point of
    its edge (mean value theorem); likewise y and z.  So each component of grad I(p) - grad phi(p) is at most
    sup |phi_a(q) - phi_a(p)| over the cell <= M sqrt(3) h, M the largest spectral norm of phi's second derivative
    (Hessian) over the cell and sqrt(3) h the cell's diagonal; the vector is at most sqrt(3) times that: 3 h M.  The field
    is a distance, |grad phi| = 1, so the angle is at most asin(3 h M).  Where one plane is nearest, M = 0.  Where the
    sphere is nearest, the Hessian of |q - c| has eigenvalues 0, 1/rho, 1/rho: M = 1 / (rho(p) - sqrt(3) h), rho the
    distance from the sphere's centre.  This holds in a cell in which phi is one smooth branch: the branch that is least
    at the cell's lowest corner is least by more than 2 sqrt(3) h there (every branch is 1-Lipschitz), |.| has no kink in the
    cell (a plane's inner value, which is linear, has one sign at the eight corners; the sphere's is further than
    sqrt(3) h from 0 at the lowest corner), and no corner is clamped.
    float32 adds: a gradient component comes from eight stored values and fewer than 32 roundings, each at most 2^-24
    for values in [-1, 1]; against a gradient of h / trunc per voxel that is an angle of at most
    sqrt(3) 32 2^-24 trunc / h, plus 8 2^-24 for the length and the three quotients."""
    g = tc.ROOM_VOLUME
    h, trunc = g["voxel"], g["trunc"]
    vol = tsdf_model.Volume(g["dims"], h, g["origin"], trunc)
    cx, cy, cz = (c.astype(np.float64) for c in vol.centres())
    Z, Y, X = np.meshgrid(cz, cy, cx, indexing="ij")
    phi = tc.room_distance(np.array([X.ravel(), Y.ravel(), Z.ravel()])).reshape(X.shape)
    vol.tsdf[:] = np.minimum(phi / trunc, 1.0).astype(np.float32)
    vol.weight[:] = 1
    depth, truth = tc.room_frame(*tc.ROOM_FOURTH)
    pose = truth.copy()
    pose[:3, 3] += (0.13, -0.13, -0.13)
    params = binding.default_sdf_params(fx=tc.ROOM_FX, cx=tc.ROOM_CX)
    vp = binding.tsdf_params(dims=g["dims"], voxel=h, origin=g["origin"], trunc=trunc)
    cell, value, terms, accepted = binding.sdf_pixels(params, vp, pose, depth, vol.tsdf, vol.weight, terms=True)
    model = sm.pixels(depth, tc.ROOM_FX, tc.ROOM_CX, vol, pose, normals=True)
    assert cell.tobytes() == model["cell"].tobytes() and value.tobytes() == model["value"].tobytes()
    ok = (cell >= 0) & (value != 0)
    # the normal the host function used: terms[24 + a] = n_a D, a product of two floats, exact in double
    n = (terms[ok, 24:27] / value[ok].astype(np.float64)[:, None]).T
    assert np.array_equal(n.astype(np.float32), model["normal"][:, ok])
    p = model["point"][:, ok].astype(np.float64)
    dims = g["dims"]
    at = cell[ok].astype(np.int64)
    corner = np.array([cx[at % dims[0]], cy[(at // dims[0]) % dims[1]], cz[at // (dims[0] * dims[1])]])
    diag = np.sqrt(3.0) * h
    inner, _, _ = room_branches(corner)
    order = np.argsort(np.abs(inner), axis=0)
    k = order[0]
    cols = np.arange(k.size)
    least, second = np.abs(inner)[k, cols], np.abs(inner)[order[1], cols]
    # all eight corners: none clamped; a plane's inner value is linear, so one sign at the corners is one sign in the cell
    one_sign, unclamped = np.ones(k.size, bool), np.ones(k.size, bool)
    for e in range(8):
        q = corner + h * np.array([[e & 1], [(e >> 1) & 1], [e >> 2]])
        inner_q = room_branches(q)[0]
        one_sign &= np.sign(inner_q[k, cols]) == np.sign(inner[k, cols])
        unclamped &= np.abs(inner_q).min(0) < trunc
    no_kink = np.where(k == 3, least > diag, one_sign & (least > 0))
    smooth = (second - least > 2 * diag) & no_kink & unclamped
    inner_p, grads_p, rho_p = room_branches(p)
    assert (np.argmin(np.abs(inner_p), axis=0)[smooth] == k[smooth]).all()
    truth_n = grads_p[k, :, cols].T  # (3, n): the analytic gradient at p, of the branch of the cell
    cosang = np.clip((n * truth_n).sum(0) / np.linalg.norm(n, axis=0), -1, 1)
    angle = np.arccos(cosang)
    float_term = np.sqrt(3.0) * 32 * 2.0 ** -24 * trunc / h + 8 * 2.0 ** -24
    M = np.where(k == 3, 1.0 / np.maximum(rho_p - diag, 1e-9), 0.0)
    bound = np.arcsin(np.minimum(3 * h * M, 1.0)) + float_term
    flat, ball = smooth & (k != 3), smooth & (k == 3)
    print(f"accepted {accepted}, in one smooth branch {int(smooth.sum())}: planes {int(flat.sum())}, sphere {int(ball.sum())}")
    print(f"planes: largest angle {np.degrees(angle[flat].max()):.3e} deg, bound {np.degrees(float_term):.3e} deg")
    print(f"sphere: largest angle {np.degrees(angle[ball].max()):.3f} deg, its bound {np.degrees(bound[ball][np.argmax(angle[ball])]):.3f} deg; "
          f"largest bound {np.degrees(bound[ball].max()):.3f} deg, smallest {np.degrees(bound[ball].min()):.3f} deg")
    assert flat.sum() > 1000 and ball.sum() > 100
    assert (angle[smooth] <= bound[smooth]).all()
