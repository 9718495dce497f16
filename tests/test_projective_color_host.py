"""K26 without a device: the three host-only functions -- icpk_intensity_pyramid_host (csrc/pyramid_rule.h),
icpk_raycast_color_gradients_host (csrc/raycast_color_rule.h) and icpk_projective_pixels_colored
(csrc/projective_rule.h), each compiled from the header its kernel includes -- against tests/projective_color_model.py
byte for byte on the cases of tests/projective_color_cases.py; the properties the rules state; the refusals; and the
wall the feature is for, settled on the numpy models before anything runs on a device."""
import ctypes as C

import numpy as np
import pytest

import color_model as cm
import gicp_model
import projective_cases as pc
import projective_color_cases as kc
import projective_color_model as km
import projective_model as jm
import pyramid_model as pm
from icp_slam_prototype_amd import binding, build, depth, synth


@pytest.fixture(scope="module")
def lib():
    build.build()
    return binding.load()


def params_of(c, **kw):
    return binding.default_projective_params(**dict(dict(level=c["level"], fx=c["fx"], cx=c["cx"], max_dist=c["max_dist"],
                                                         min_normal_cos=c["min_normal_cos"]), **kw))


# ---- the intensity pyramid --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", kc.PYRAMID_CASES)
def test_intensity_pyramid_host_gives_the_models_bytes(lib, name):
    d, inten, K, levels = kc.pyramid_case(name)
    want = kc.pyramid_expected(name)
    p = depth.pyramid_params(levels=levels, range_cutoff=K)
    masks = pm.pyramid(d, levels, K)
    for l in range(levels):
        got = binding.intensity_pyramid_host(d, inten, l, p)
        assert got.shape == want[l].shape and got.tobytes() == want[l].tobytes(), (name, l)
        assert got.min() >= 0.0 and got.max() <= 1.0
        assert l == 0 or not got[masks[l] == 0].any()  # the validity mask is the depth level's (level 0 is the input)


def test_the_properties_the_rule_states(lib):
    # K = 1 is plain subsampling up to the quantisation wherever no neighbour has the centre's very depth (with K = 1 a
    # tap counts iff its depth EQUALS the centre's: the depth then averages to itself, the intensity does not)
    d, inten, K, levels = kc.pyramid_case("cutoff_1")
    assert K == 1
    want = kc.pyramid_expected("cutoff_1")
    ds = pm.pyramid(d, levels, K)
    for l in range(1, levels):
        below, mask = want[l - 1][::2, ::2], ds[l] != 0
        sub = (np.rint(below.astype(np.float64) * 32768.0) / 32768.0).astype(np.float32)
        pad = np.pad(ds[l - 1].astype(np.int64), 1, constant_values=-1)
        r, c = ds[l].shape
        alone = np.ones((r, c), bool)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dy or dx:
                    alone &= pad[1 + dy:1 + dy + 2 * r - 1:2, 1 + dx:1 + dx + 2 * c - 1:2] != ds[l - 1][::2, ::2]
        assert (alone & mask).sum() > 0.5 * mask.sum()
        assert want[l][alone & mask].tobytes() == sub[alone & mask].tobytes() and not want[l][~mask].any()
    # a depth step of K is never averaged across: each side keeps its own intensity exactly
    for name in ("half_planes_odd", "half_planes_even"):
        d, inten, K, levels = kc.pyramid_case(name)
        ds = pm.pyramid(d, levels, K)
        for l, got in enumerate(kc.pyramid_expected(name)):
            inner = np.ones(got.shape, bool)
            if l == 0:
                inner[0, 0] = inner[-1, -1] = False  # (the two pixels that carry the ends of the range)
            else:
                inner[0, :2] = inner[-2:, -2:] = False  # ... and what they spread into on their own side of the step
                inner[:2, 0] = False
            near = ds[l] == 4000
            assert set(np.unique(got[inner & near])) <= {np.float32(0.25)} and set(np.unique(got[inner & ~near])) <= {np.float32(0.75)}


def test_intensity_pyramid_refusals(lib):
    d, inten, K, levels = kc.pyramid_case("3x3")
    E = binding.E_ARG

    def code(dd=d, ii=inten, level=1, **kw):
        try:
            binding.intensity_pyramid_host(dd, ii, level, depth.pyramid_params(**dict(dict(levels=3), **kw)))
        except binding.IcpkError as e:
            return e.code
        return 0

    assert code() == 0 and code(level=2) == 0
    assert code(level=3) == E and code(level=-1) == E and code(levels=0) == E and code(levels=9) == E
    assert code(range_cutoff=0) == E and code(range_cutoff=65537) == E
    for bad in (np.nan, np.inf, -1e-6, 1.0001):
        ii = np.array(inten)
        ii[1, 2] = bad
        assert code(ii=ii) == E, bad
    assert lib.icpk_intensity_pyramid_host(None, None, None, 3, 3, 0, None) == E
    out = np.zeros(9, np.float32)
    fp, u16 = C.POINTER(C.c_float), C.POINTER(C.c_uint16)
    assert lib.icpk_intensity_pyramid_host(None, d.ctypes.data_as(u16), np.array(inten).ctypes.data_as(fp), 0, 3, 0, out.ctypes.data_as(fp)) == E


# ---- the view gradients -----------------------------------------------------------------------------------------------
def test_the_gradient_cases_hold_their_conditions():
    kc.check_gradient_conditions()


@pytest.mark.parametrize("name", kc.GRADIENT_CASES)
def test_view_gradients_host_gives_the_models_bytes(lib, name):
    c = kc.gradient_case(name)
    S, g, n = binding.raycast_color_gradients_host(c["maps"], c["radius"], c["min_neighbors"])
    assert S.tobytes() == c["sums"].tobytes()
    want = c["gradients"].reshape(3, -1).T
    assert g.tobytes() == np.ascontiguousarray(want).tobytes()
    assert n == int((want != 0).any(1).sum())
    # color_model.gradients_from_sums serves unchanged on the sums
    again = cm.gradients_from_sums(S, c["maps"][3:6].reshape(3, -1), c["radius"], c["min_neighbors"])
    assert again.tobytes() == c["gradients"].reshape(3, -1).tobytes()


def test_view_gradients_on_a_view_no_ray_cast_gives(lib):
    """hit pixels with the zero normal and a non-unit one (m kept, nine zero sums, no gradient), holes among the
    neighbours, a NaN point; and windows at the start, inside and at the last pixel"""
    maps = kc.synthetic_view()
    rows, cols = maps.shape[1:]
    g_want, S_want = km.view_gradients(maps, 0.05, 3)
    S, g, n = binding.raycast_color_gradients_host(maps, 0.05, 3)
    assert S.tobytes() == S_want.tobytes() and g.tobytes() == np.ascontiguousarray(g_want.reshape(3, -1).T).tobytes()
    at = lambda r, c: r * cols + c
    for r, c in ((4, 5), (2, 2)):
        assert S[at(r, c), 0] >= 1 and not S[at(r, c), 1:].any() and not g[at(r, c)].any()
    assert S[at(6, 7), 0] == 0 and not g[at(6, 7)].any()
    assert n > 0 and ((S[:, 0] > 1) & (S[:, 0] < 9) & (maps[6].reshape(-1) > 0)).any()
    for first, count in ((0, 1), (0, 7), (40, 13), (rows * cols - 1, 1), (rows * cols, 0)):
        Sw, gw, _ = binding.raycast_color_gradients_host(maps, 0.05, 3, first=first, count=count)
        assert Sw.tobytes() == S[first:first + count].tobytes() and gw.tobytes() == g[first:first + count].tobytes()


def test_view_gradient_refusals(lib):
    maps = kc.synthetic_view()
    E = binding.E_ARG

    def code(radius=0.05, min_nb=3, **kw):
        try:
            binding.raycast_color_gradients_host(maps, radius, min_nb, **kw)
        except binding.IcpkError as e:
            return e.code
        return 0

    assert code() == 0
    for r in (0.0, -1.0, np.nan, np.inf):
        assert code(radius=r) == E
    assert code(min_nb=0) == E and code(first=-1) == E and code(count=-1) == E and code(first=98, count=2) == E
    assert lib.icpk_raycast_color_gradients_host(None, 9, 11, 0.05, 3, 0, 1, None, None) == E
    fp = C.POINTER(C.c_float)
    planes = (fp * 8)(*[maps[k].ctypes.data_as(fp) for k in range(7)], None)
    assert lib.icpk_raycast_color_gradients_host(planes, 9, 11, 0.05, 3, 0, 1, None, None) == E
    planes[7] = maps[7].ctypes.data_as(fp)
    assert lib.icpk_raycast_color_gradients_host(planes, 9, 11, 0.05, 3, 0, 99, None, None) >= 0  # (both outputs may be NULL)
    assert lib.icpk_raycast_color_gradients_host(planes, 0, 11, 0.05, 3, 0, 0, None, None) == E


# ---- the joint terms --------------------------------------------------------------------------------------------------
def host(name, lam=cm.LAMBDA, **kw):
    c = kc.case(name)
    v = c["view"]
    return binding.projective_pixels_colored(params_of(c), c["estimate"], c["level_image"], kc.maps_of(name), v["shape"], v["fx"],
                                             v["cx"], c["view_pose"], c["level_intensity"], kc.gradients_of(name),
                                             color=dict(lambda_geometric=lam), terms=True, **kw)


def test_the_cases_accept_what_k25_accepts():
    kc.check_conditions()
    assert kc.case("260x260")["level_image"].size > 256 * 256 and kc.case("room_l1")["level_intensity"].shape == (60, 80)
    assert binding.default_projective_color_params().lambda_geometric == np.float32(0.968)
    assert C.sizeof(binding.ProjectiveColorParams) == 4


@pytest.mark.parametrize("name", kc.NAMES)
def test_colored_host_function_gives_the_models_bytes(lib, name):
    lambdas = kc.LAMBDAS if name in ("room_l1", "7x9", "260x260", "normal_gate") else (cm.LAMBDA,)
    k25 = pc.expected(name)
    for lam in lambdas:
        want = kc.expected(name, lam)
        pixel, dist, terms, pairs = host(name, lam)
        assert pairs == want["count"] == k25["count"]
        assert pixel.tobytes() == k25["pixel"].tobytes() and dist.tobytes() == k25["dist"].tobytes()  # counts and codes are K25's
        assert terms.tobytes() == want["terms"].tobytes(), lam
        assert gicp_model.canonical(terms).tobytes() == want["sums"].tobytes()
        assert terms[:, 27].tobytes() == k25["terms"][:, 27].tobytes()


@pytest.mark.parametrize("name", ("room_l1", "17x19", "260x260", "normal_gate"))
def test_lambda_one_is_the_geometric_step_bit_for_bit(lib, name):
    c = kc.case(name)
    v = c["view"]
    pixel, dist, terms, _ = host(name, 1.0)
    gp, gd, gt, _ = binding.projective_pixels(params_of(c), c["estimate"], c["level_image"], kc.maps_of(name), v["shape"], v["fx"],
                                              v["cx"], c["view_pose"], terms=True)
    assert pixel.tobytes() == gp.tobytes() and dist.tobytes() == gd.tobytes() and terms.tobytes() == gt.tobytes()
    assert gicp_model.canonical(terms).tobytes() == kc.expected_geometric(name)["sums"].tobytes()
    # ... and lambda = 0.5 is not
    assert host(name, 0.5)[2].tobytes() != gt.tobytes()


def test_a_window_and_the_refusals_of_the_colored_host_function(lib):
    want = kc.expected("normal_gate")
    first, count = 160 * 37 + 11, 1000
    pixel, dist, terms, pairs = host("normal_gate", first=first, count=count)
    sl = slice(first, first + count)
    assert pixel.tobytes() == want["pixel"][sl].tobytes() and terms.tobytes() == want["terms"][sl].tobytes()
    assert pairs == int((want["pixel"][sl] >= 0).sum())
    assert host("room_l0", first=19200, count=0)[3] == 0 and host("room_l0", first=19199, count=1)[0].size == 1
    E = binding.E_ARG
    for lam in (np.nan, np.inf, -0.001, 1.001):
        with pytest.raises(binding.IcpkError) as e:
            host("7x9", lam)
        assert e.value.code == E
    c = kc.case("7x9")
    for kw in (dict(level=-1), dict(fx=0.0), dict(max_dist=0.0), dict(min_pairs=0), dict(max_iterations=65)):
        v = c["view"]
        with pytest.raises(binding.IcpkError) as e:
            binding.projective_pixels_colored(params_of(c, **kw), c["estimate"], c["level_image"], kc.maps_of("7x9"), v["shape"],
                                              v["fx"], v["cx"], c["view_pose"], c["level_intensity"], kc.gradients_of("7x9"))
        assert e.value.code == E, kw
    p = params_of(c)
    assert lib.icpk_projective_pixels_colored(C.byref(p), None, None, 7, 9, None, 120, 160, 1.0, 1.0, None, 0, 1, None, None, None,
                                              None, None, None, None) == E
    lib.icpk_default_projective_color_params(None)  # (nothing happens)
    for f in (lib.icpk_projective_reduce_colored, lib.icpk_align_projective_colored):
        assert f(None, None, None, None, None, None) == E
    assert lib.icpk_depth_pyramid_set_intensity(None, None, 1, 1) == E and lib.icpk_depth_pyramid_get_intensity(None, 0, None) == E
    assert lib.icpk_tsdf_raycast_color_gradients(None, 0.1, 4, 0) == E
    assert lib.icpk_tsdf_get_raycast_color_gradients(None, None, None, None) == E
    assert lib.icpk_tsdf_get_raycast_color_gradient_sums(None, None) == E


# ---- the room, on the models ------------------------------------------------------------------------------------------
def test_the_room_basin_on_the_models():
    """K25's basin table on room_color with the numpy models, geometric and coloured side by side, printed for DESIGN.md
    (the device gives the same digits: tests/test_gpu_projective_color.py).  The geometric column meets K25's quarter-voxel
    bar at every s.  The coloured one does NOT from s = 2 on (462, 733 and 966 mm: lost) -- the room's texture is step
    edges through 62.5 mm voxels -- so nothing is asserted on it beyond s = 1, where it is the better of the two.  (K25's
    tracking table, which builds a volume per tracker, was run with the same models outside the suite: geometric 3.83 /
    8.28 / 7.15 mm, coloured 4.55 / 5.58 / 6.71 mm after frames 1, 2, 3.)"""
    import tsdf_cases as tc
    import tsdf_raycast_cases as rc

    (r3, t3), (r4, t4) = tc.ROOM_MOTIONS[2], tc.ROOM_FOURTH
    P3 = tc.pose(r3, t3)
    voxel = tc.ROOM_VOLUME["voxel"]
    view = rc.ROOM_VIEW
    maps = kc._maps("room_color", P3, view)
    g, _ = km.view_gradients(maps, 2 * voxel, 4)
    err = lambda T, truth: float(np.linalg.norm((np.linalg.inv(truth) @ T)[:3, 3]))
    rows = []
    for s in (1, 2, 3, 4):
        rot = tuple(a + s * (b - a) for a, b in zip(r3, r4))
        shift = tuple(a + s * (b - a) for a, b in zip(t3, t4))
        d, truth = tc.room_frame(rot, shift)
        geo = dict(fx_s=np.float32(tc.ROOM_FX), cx_s=np.float32(tc.ROOM_CX), view=maps, view_shape=view["shape"], fx_v=view["fx"],
                   cx_v=view["cx"], view_pose=P3, pose=P3, max_dist=0.5)
        a = jm.align(level=d, max_iterations=19, **geo)
        b = km.align(max_iterations=19, level=d, level_intensity=tc.room_intensity(rot, shift), gradient=g, **geo)
        rows.append((err(a["pose"], truth), err(b["pose"], truth)))
        print(f"s = {s}: geometric {1000 * rows[-1][0]:.2f} mm; coloured {1000 * rows[-1][1]:.2f} mm")
    assert all(r[0] < voxel / 4 for r in rows)
    assert rows[0][1] < rows[0][0] < voxel / 4


# ---- the wall, on the models ------------------------------------------------------------------------------------------
def test_textured_wall_frames():
    w = kc.wall()
    (d0, i0), (d1, i1) = w["frames"]
    assert d0.shape == i0.shape == kc.WALL_SHAPE and d0.dtype == np.uint16 and i0.dtype == np.float32
    assert (d0 == 5000).all() and (d1 == 4980).all()  # an exact plane, fronto-parallel, 4 mm nearer in frame 1
    assert 0.05 <= i0.min() and i0.max() <= 0.95 and i0.std() > 0.1
    # the intensity is the texture of the wall point a pixel sees
    r, c = 17, 61
    x, y = (c - kc.WALL_CX) / kc.WALL_FX, (r - kc.WALL_CX) / kc.WALL_FX
    assert abs(i0[r, c] - kc.texture(x, y)) < 1e-6
    # relief bends the wall and leaves no border
    (dr, ir), = synth.textured_wall_frames([np.eye(4)], 30, 40, fx=30.0, z=1.0, relief=0.02)
    assert dr.min() >= 4890 and dr.max() <= 5110 and len(np.unique(dr)) > 20 and (dr > 0).all()
    with pytest.raises(ValueError):
        synth.textured_wall_frames([np.diag([1.0, -1.0, -1.0, 1.0])], 30, 40)


def test_the_wall_on_the_models():
    """The claim: on an exact fronto-parallel plane the geometric projective step is degenerate (or slides), the coloured
    one recovers the in-plane motion.  The model's figures are recorded in projective_color_cases.WALL_MEASURED; the
    assertion is twice those figures, and the condition that the translation error is below a quarter of the in-plane
    motion (9 mm).  Measured: rotation (Frobenius) 5.54e-4, translation 4.98 mm of 36.3 mm; the residual lies in the
    plane, (-3.1, -3.9) mm, a quarter of the 16.7 mm a pixel covers: the volume fuses the intensity of the NEAREST pixel
    of a voxel's projection."""
    m = kc.wall_model()
    assert (m["maps"][6] > 0).sum() > 3000
    share = float((m["gradients"] != 0).any(0)[m["maps"][6] > 0].mean())
    col = m["colored"]
    rot, trans = kc.wall_errors(col["pose"])
    start = kc.wall_errors(kc.wall()["poses"][0])
    print(f"wall, model: hit pixels with a gradient {share:.3f}; start {start[0]:.3e} / {1000 * start[1]:.2f} mm; coloured "
          f"{rot:.6e} / {1000 * trans:.4f} mm after {col['iterations']} iterations")
    assert col["status"] == jm.OK and col["iterations"] == kc.WALL_ITER
    assert kc.WALL_MEASURED[1] < kc.WALL_CONDITION  # the condition, on the recorded figure
    assert rot <= 2 * kc.WALL_MEASURED[0] and trans <= 2 * kc.WALL_MEASURED[1]
    assert abs(rot - kc.WALL_MEASURED[0]) < 1e-6 and abs(trans - kc.WALL_MEASURED[1]) < 1e-6  # (the record is this model's)
    # the gap: the geometric step on the same inputs
    geo = m["geometric"]
    truth = kc.wall()["poses"][1]
    in_plane = float(np.linalg.norm(geo["pose"][:2, 3] - truth[:2, 3]))
    print(f"wall, model: geometric status {geo['status']}, iterations {geo['iterations']}, in-plane error {1000 * in_plane:.2f} mm")
    assert geo["status"] == jm.W_DEGENERATE or in_plane > 0.5 * float(np.hypot(0.030, 0.020))
