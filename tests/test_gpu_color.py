"""Colored ICP on the device (include/icpk.h, K17): the integer sums and the gradients of
icpk_estimate_target_color_gradients and the 28 sums of the joint step against the numpy model (tests/color_model.py)
bit for bit, the loop in every NN mode with the device and the host loop, the lifetime of the colours and the errors."""
import numpy as np
import pytest

import color_model as cm
import tsdf_cases
from icp_slam_prototype_amd import binding, build, synth

pytestmark = pytest.mark.gpu

P2L = binding.SOLVE_POINT_TO_PLANE
MODES = (binding.NN_EXACT, binding.NN_FILTERED, binding.NN_PRUNED, binding.NN_GRID)


@pytest.fixture(scope="module")
def ctx():
    build.build()
    c = binding.Context(0)
    yield c
    c.close()


def _code(fn, *a, **kw):
    """the status of a call through the binding: its return value, or the code of the error it raises"""
    try:
        r = fn(*a, **kw)
    except binding.IcpkError as e:
        return e.code
    if isinstance(r, tuple) and len(r) == 3:  # (T, stats, rc)
        return r[2]
    return r if isinstance(r, int) else 0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _unit(rng, k):
    v = rng.normal(size=(3, k))
    return (v / np.linalg.norm(v, axis=0)).astype(np.float32)


# ----------------------------------------------------------------------------------------------------- gradients --
def _patch(n, seed):
    """n points on a bumpy patch whose density gives a radius of 0.04 some tens of neighbours at n = 3000 and few or none
    at the small sizes; normals near +z; from 65 points on: duplicates, non-finite points, points without a normal, a
    non-unit and a non-finite host normal"""
    rng = np.random.default_rng(seed)
    side = 0.5 if n > 100 else 0.08
    pts = np.stack([rng.uniform(0, side, n), rng.uniform(0, side, n), 1 + rng.normal(0, 0.004, n)]).astype(np.float32)
    nrm = np.stack([rng.normal(0, 0.1, n), rng.normal(0, 0.1, n), np.ones(n)])
    nrm = (nrm / np.linalg.norm(nrm, axis=0)).astype(np.float32)
    inten = rng.uniform(0, 1, n).astype(np.float32)
    if n >= 65:
        pts[:, 10:14] = pts[:, 20:24]               # duplicates (with other intensities)
        pts[:, 30] = np.float32([np.nan, 0.1, 1])   # non-finite points
        pts[1, 31] = np.float32(np.inf)
        nrm[:, 40:45] = 0                           # no normal
        nrm[:, 45] = np.float32([0, 0, 3])          # a non-unit host normal
        nrm[:, 46] = np.float32([np.nan, 0, 1])
        nrm[:, 47] = np.float32([0, 0, 1.002])      # outside [1 - 2^-10, 1 + 2^-10] by a little
        nrm[:, 48] = np.float32([0, 0, 1.0002])     # inside
        inten[50], inten[51] = 0.0, 1.0
    return pts, nrm, inten


def _estimate(ctx, pts, nrm, inten, radius, min_nb):
    ctx.set_target(pts)
    ctx.set_target_normals(nrm)
    ctx.set_target_colors(inten)
    ctx.estimate_target_color_gradients(radius, min_nb, keep_sums=True)
    return ctx.get_target_color_gradients(), ctx.color_gradient_sums()


@pytest.mark.parametrize("n", [1, 7, 9, 65, 3001])
def test_gradient_sums_and_gradients(ctx, n):
    pts, nrm, inten = _patch(n, n)
    radius, min_nb = 0.04, 4
    g, S = _estimate(ctx, pts, nrm, inten, radius, min_nb)
    wg, wS = cm.gradients(pts, nrm, inten, radius, min_nb)
    assert np.array_equal(S, wS)
    assert np.array_equal(_bits(g), _bits(wg))
    if n >= 65:
        assert not S[30].any() and not S[31].any()                       # a non-finite point: an empty neighbourhood
        assert S[40:48, 0].all() and not S[40:48, 1:].any() and not g[:, 40:48].any()  # no usable normal: m only
        assert S[48, 1:].any()
    if n > 3000:
        assert (g != 0).any(0).mean() > 0.9 and S[:, 0].max() > 40
    # the same bits on a second run and for another order of the cloud
    g2, S2 = _estimate(ctx, pts, nrm, inten, radius, min_nb)
    assert np.array_equal(S2, S) and np.array_equal(_bits(g2), _bits(g))
    perm = np.random.default_rng(n + 1).permutation(n)
    gp, Sp = _estimate(ctx, pts[:, perm], nrm[:, perm], inten[perm], radius, min_nb)
    assert np.array_equal(Sp, S[perm]) and np.array_equal(_bits(gp), _bits(g[:, perm]))
    # min_neighbors above every m: no gradient anywhere, the sums as before
    g0, S0 = _estimate(ctx, pts, nrm, inten, radius, int(S[:, 0].max()) + 1)
    assert np.array_equal(S0, S) and not g0.any()


def test_gradients_on_a_lattice_with_pairs_at_exactly_the_radius(ctx):
    w = synth.lattice_wall(rows=30, cols=40)
    pts = w["target"]
    n = pts.shape[1]
    radius = np.float32(3) * np.float32(0.01)  # three lattice steps
    d = cm.nm.pair_dist(pts[:, :1].repeat(n, 1), pts)
    assert (d == radius).sum() >= 2  # (the rule's `<=` decides these)
    rng = np.random.default_rng(11)
    nrm = np.tile(np.float32([[0], [0], [-1]]), (1, n))
    inten = (0.5 + 0.3 * np.sin(pts[0] * 20) * np.cos(pts[1] * 15)).astype(np.float32)
    g, S = _estimate(ctx, pts, nrm, inten, radius, 4)
    wg, wS = cm.gradients(pts, nrm, inten, radius, 4)
    assert np.array_equal(S, wS) and np.array_equal(_bits(g), _bits(wg))
    # (29 lattice points lie within three steps; whether the four at exactly three count is the float compare's word)
    assert 25 <= S[:, 0].max() <= 29 and (g != 0).any(0).mean() > 0.95 and not g[2].any()
    perm = rng.permutation(n)
    gp, Sp = _estimate(ctx, pts[:, perm], nrm[:, perm], inten[perm], radius, 4)
    assert np.array_equal(Sp, S[perm]) and np.array_equal(_bits(gp), _bits(g[:, perm]))


# ---------------------------------------------------------------------------------------------------------- hook --
@pytest.fixture(scope="module")
def scene():
    """a target with unit and zero normals, intensities and -- from the device, checked against the model here once --
    gradients, zero ones among them; in a context of its own that keeps it"""
    build.build()
    rng = np.random.default_rng(0)
    nt = 2000
    tgt = (rng.uniform(-1, 1, (3, nt)) + 5).astype(np.float32)
    tn = _unit(rng, nt)
    tn[:, rng.random(nt) < 0.2] = 0
    tc = rng.uniform(0, 1, nt).astype(np.float32)
    c = binding.Context(0)
    c.set_target(tgt)
    c.set_target_normals(tn)
    c.set_target_colors(tc)
    c.estimate_target_color_gradients(0.3, 28)
    g = c.get_target_color_gradients()
    wg, _ = cm.gradients(tgt, tn, tc, 0.3, 28)
    assert np.array_equal(_bits(g), _bits(wg))
    has = (g != 0).any(0)
    assert 0.2 < has[(tn != 0).any(0)].mean() < 0.9  # gradients and zero gradients on points with a normal
    yield dict(ctx=c, tgt=tgt, tn=tn, tc=tc, g=g)
    c.close()


@pytest.mark.parametrize("n", [1, 200, 255, 256, 257, 3000, 65536, 70001])
def test_hook_sizes_and_lambdas(scene, n):
    """1, several and 256 blocks (and more than one element per lane); zero normals and zero gradients mixed in; the
    working source at the uploaded pose and moved; lambda_geometric 0, 0.5, 0.968 and 1"""
    c, tgt, tn, tc, g = (scene[k] for k in ("ctx", "tgt", "tn", "tc", "g"))
    rng = np.random.default_rng(n)
    src = (tgt[:, rng.integers(0, tgt.shape[1], n)] + rng.normal(0, 0.03, (3, n))).astype(np.float32)
    sc = rng.uniform(0, 1, n).astype(np.float32)
    c.set_source(src)
    c.set_source_colors(sc)
    R = synth.rot_xyz_deg(0.3, -0.2, 0.4).astype(np.float32)
    for mode, moved in ((binding.NN_GRID, True), (binding.NN_EXACT, False)):
        c.reset_source()
        if moved:
            c.transform_source(R, np.float32([0.004, -0.003, 0.002]))
        cur = c.get_source()
        idx, dist = c.nn(mode)
        for lam in (0.0, 0.5, 0.968, 1.0):
            c.set_colored(False, lam)
            got, cnt = c.reduce_colored(0.06)
            want, wcnt = cm.sums(cur, tgt, tn, g, tc, sc, idx, dist, 0.06, lam)
            assert cnt == wcnt and (n < 200 or 0 < cnt < n)
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (n, mode, lam)
        plain, pcnt = c.reduce_p2l(0.06)  # (lambda_geometric is 1 here)
        assert pcnt == cnt and np.array_equal(plain.view(np.uint64), got.view(np.uint64))
    c.set_colored(False, 0.968)


# ---------------------------------------------------------------------------------------------------------- loop --
@pytest.fixture(scope="module")
def wall():
    return cm.wall_pair()


def _install(ctx, p):
    ctx.set_target(p["target"])
    ctx.set_target_normals(p["target_normals"])
    ctx.set_target_colors(p["target_intensity"])
    ctx.set_source(p["source"])
    ctx.set_source_colors(p["source_intensity"])
    ctx.estimate_target_color_gradients(cm.WALL_RADIUS, cm.WALL_MIN_NB)


def _run(ctx, **kw):
    T, st, rc = ctx.align(solve=P2L, max_nn_dist=cm.WALL_MAX_DIST, **kw)
    idx, dist = ctx.get_associations()
    return dict(T=T.copy(), rc=rc, stats=(st.iterations, st.status, st.final_pairs, np.float32(st.final_mse).tobytes()),
                idx=idx.copy(), dist=dist.copy(), src=ctx.get_source().copy(), trace=ctx.get_trace())


def _assert_same(a, b, what):
    assert a["rc"] == b["rc"] and a["stats"] == b["stats"], (what, a["stats"], b["stats"])
    for k in ("T", "dist", "src"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)
    assert np.array_equal(a["idx"], b["idx"]), what
    assert len(a["trace"]) == len(b["trace"]) == a["stats"][0], what
    for x, y in zip(a["trace"], b["trace"]):
        assert x["R"].tobytes() == y["R"].tobytes() and x["t"].tobytes() == y["t"].tobytes(), what
        assert x["n_pairs"] == y["n_pairs"] and np.float32(x["mse"]).tobytes() == np.float32(y["mse"]).tobytes(), what


def test_flat_wall_in_every_mode_and_against_the_model(ctx, wall, oracle):
    _install(ctx, wall)
    g = ctx.get_target_color_gradients()
    wg, _ = cm.gradients(wall["target"], wall["target_normals"], wall["target_intensity"], cm.WALL_RADIUS, cm.WALL_MIN_NB)
    assert np.array_equal(_bits(g), _bits(wg))
    fixed = dict(max_iterations=cm.WALL_ITER, fixed_iterations=1)
    # geometry alone: degenerate at the first step, in both loops
    ctx.set_colored(False)
    for host in (0, 1):
        T, st, rc = ctx.align(solve=P2L, host_loop=host, max_nn_dist=cm.WALL_MAX_DIST, **fixed)
        assert (rc, st.status, st.iterations) == (binding.W_DEGENERATE, binding.W_DEGENERATE, 0)
        assert T.tobytes() == np.eye(4, dtype=np.float32).tobytes()
    ctx.set_colored(True)
    ref = _run(ctx, nn_mode=binding.NN_GRID, host_loop=0, **fixed)
    assert ref["rc"] == 0 and ref["stats"][0] == cm.WALL_ITER
    for mode in MODES:
        for host in (0, 1):
            _assert_same(ref, _run(ctx, nn_mode=mode, host_loop=host, **fixed), ("fixed", mode, host))
    # threshold exit: the mse the loop saw at its 4th test ends it there, everywhere the same
    thr = float(ref["trace"][3]["mse"])
    first = None
    for mode in MODES:
        for host in (0, 1):
            r = _run(ctx, nn_mode=mode, host_loop=host, max_iterations=cm.WALL_ITER, threshold=thr)
            assert r["rc"] == 0 and 1 <= r["stats"][0] <= cm.WALL_ITER, r["stats"]
            first = first or r
            _assert_same(first, r, ("threshold", mode, host))
    ctx.set_colored(False)
    # the pose: within the bound the host test fixes (twice the model's measured errors), and the model's own
    er, et = cm.pose_errors(ref["T"], wall["T_true"])
    print("flat wall on the device: rotation", er, "translation", et)
    assert er <= 2 * cm.WALL_MEASURED[0] and et <= 2 * cm.WALL_MEASURED[1]
    m = cm.align(wall["source"], wall["target"], wall["target_normals"], g, wall["target_intensity"],
                 wall["source_intensity"], oracle, iterations=cm.WALL_ITER, max_dist=cm.WALL_MAX_DIST)
    T = ref["T"].astype(np.float64)
    err = (np.linalg.norm(T[:3, :3] - m["T"][:3, :3]), np.linalg.norm(T[:3, 3] - m["T"][:3, 3]))
    print("device against model: rotation", err[0], "translation", err[1])
    assert err[0] < 1e-5 and err[1] < 1e-5
    assert [t["n_pairs"] for t in ref["trace"]] == m["pairs"]
    assert np.array_equal(ref["idx"], m["final_idx"])
    # more than 65536 queries: a lane of K17 takes several pairs; the device loop reads the sweep's records, the host
    # loop the keys
    _install(ctx, cm.wall_pair(rows=240, cols=300))
    ctx.set_colored(True)
    few = dict(nn_mode=binding.NN_GRID, max_iterations=4, fixed_iterations=1)
    dev = _run(ctx, host_loop=0, **few)
    assert dev["rc"] == 0 and dev["stats"][0] == 4 and dev["src"].shape[1] > 65536
    _assert_same(dev, _run(ctx, host_loop=1, **few), "more than 65536 queries")
    ctx.set_colored(False)


def test_setting_off_and_other_flavours_return_todays_bytes(ctx):
    p = cm.wall_pair(relief=0.003, rows=40, cols=50)
    kw = dict(max_iterations=6, fixed_iterations=1, max_nn_dist=0.3)

    def runs(c):
        out = []
        for solve in (P2L, binding.SOLVE_KABSCH, binding.SOLVE_REFERENCE):
            T, st, rc = c.align(solve=solve, **kw)
            out.append((rc, st.iterations, st.final_pairs, np.float32(st.final_mse).tobytes(), T.tobytes(),
                        c.get_source().tobytes()))
        return out

    with binding.Context(0) as fresh:  # a context that never heard of colours
        fresh.set_target(p["target"])
        fresh.estimate_target_normals(0.035, 5)
        tn = fresh.get_target_normals()
        fresh.set_source(p["source"])
        want = runs(fresh)
    assert want[0][0] == 0
    p["target_normals"] = tn
    _install(ctx, p)
    assert runs(ctx) == want                       # the default: off
    ctx.set_colored(True)
    on = runs(ctx)
    assert on[1:] == want[1:] and on[0][0] == 0 and on[0][4] != want[0][4]  # Kabsch and reference ignore the setting
    ctx.set_colored(False)
    assert runs(ctx) == want


# ------------------------------------------------------------------------------------------ lifetime and errors --
def test_set_get_and_argument_errors(ctx):
    rng = np.random.default_rng(2)
    p = synth.kinect_pair(rows=60, cols=80, seed=5)
    src, tgt = p["source"], p["target"]
    ns, nt = src.shape[1], tgt.shape[1]
    ctx.set_target(tgt)
    ctx.set_source(src)
    sc, tc = rng.uniform(0, 1, ns).astype(np.float32), rng.uniform(0, 1, nt).astype(np.float32)
    sc[0], sc[1], tc[0], tc[1] = 0, 1, 1, 0
    ctx.set_source_colors(sc)
    ctx.set_target_colors(tc)
    assert ctx.get_source_colors().tobytes() == sc.tobytes() and ctx.get_target_colors().tobytes() == tc.tobytes()
    for setter, getter, good in ((ctx.set_source_colors, ctx.get_source_colors, sc),
                                 (ctx.set_target_colors, ctx.get_target_colors, tc)):
        assert _code(setter, good[:-1]) == binding.E_ARG
        for bad in (np.nan, np.inf, -np.inf, -1e-6, 1.0000001):
            v = good.copy()
            v[good.size // 2] = bad
            assert _code(setter, v) == binding.E_ARG, bad
        assert getter().tobytes() == good.tobytes()  # (nothing changed)
    # the gradient estimate: what it needs, and its arguments
    assert _code(ctx.estimate_target_color_gradients, 0.05) == binding.E_NOT_SET  # (no normals)
    assert _code(ctx.get_target_color_gradients) == binding.E_NOT_SET
    ctx.set_target_normals(_unit(rng, nt))
    lib, h = ctx._lib, ctx._h
    for radius, mn, flags in ((0.0, 4, 0), (-1.0, 4, 0), (float("inf"), 4, 0), (float("nan"), 4, 0), (0.05, 0, 0), (0.05, 4, 2)):
        assert lib.icpk_estimate_target_color_gradients(h, radius, mn, flags) == binding.E_ARG
    assert _code(ctx.get_target_color_gradients) == binding.E_NOT_SET
    ctx.estimate_target_color_gradients(0.05, 4)
    assert ctx.get_target_color_gradients().shape == (3, nt)
    assert _code(ctx.color_gradient_sums) == binding.E_NOT_SET  # (not kept)
    ctx.estimate_target_color_gradients(0.05, 4, keep_sums=True)
    assert ctx.color_gradient_sums().shape == (nt, 10)
    with binding.Context(0) as fresh:
        assert _code(fresh.set_source_colors, sc) == binding.E_NOT_SET
        assert _code(fresh.set_target_colors, tc) == binding.E_NOT_SET
        assert _code(fresh.get_source_colors) == binding.E_NOT_SET
        assert _code(fresh.get_target_colors) == binding.E_NOT_SET
        assert _code(fresh.estimate_target_color_gradients, 0.05) == binding.E_NOT_SET
        fresh.set_target(tgt)
        fresh.set_target_normals(_unit(rng, nt))
        assert _code(fresh.estimate_target_color_gradients, 0.05) == binding.E_NOT_SET  # (no colours)
    # lambda_geometric: finite and in [0, 1], else the setting stays
    ctx.set_colored(False, 0.25)
    ctx.nn(binding.NN_GRID, fetch=False)
    keep = ctx.reduce_colored(0.3)[0]
    for bad in (-1e-6, 1.0000001, float("nan"), float("inf")):
        assert _code(ctx.set_colored, True, bad) == binding.E_ARG
        assert np.array_equal(ctx.reduce_colored(0.3)[0].view(np.uint64), keep.view(np.uint64))
    # ... and it stayed off: point-to-plane is the plain one
    a = ctx.align(solve=P2L, max_iterations=2, fixed_iterations=1)
    ctx.set_colored(False, 1.0)
    b = ctx.align(solve=P2L, max_iterations=2, fixed_iterations=1)
    assert a[0].tobytes() == b[0].tobytes()
    ctx.set_colored(False, 0.968)
    # the host helper
    bgr = rng.integers(0, 256, (50, 3)).astype(np.uint8)
    bgr[0], bgr[1] = 0, 255
    want = ((bgr[:, 0].astype(np.float64) + bgr[:, 1] + bgr[:, 2]) / 765.0).astype(np.float32)
    assert binding.intensity_from_bgr(bgr).tobytes() == want.tobytes() and want[0] == 0 and want[1] == 1


def test_alignment_errors(ctx, wall):
    small = cm.wall_pair(rows=20, cols=30)

    def install(source_colors=True, target_colors=True, gradients=True, normals=True):
        ctx.set_target(small["target"])
        ctx.set_source(small["source"])
        if normals:
            ctx.set_target_normals(small["target_normals"])
        if target_colors:
            ctx.set_target_colors(small["target_intensity"])
        if source_colors:
            ctx.set_source_colors(small["source_intensity"])
        if gradients and normals and target_colors:
            ctx.estimate_target_color_gradients(cm.WALL_RADIUS, cm.WALL_MIN_NB)

    ctx.set_colored(True)
    try:
        for missing in ("source_colors", "target_colors", "gradients", "normals"):
            install(**{missing: False})
            assert _code(ctx.align, solve=P2L, max_iterations=2) == binding.E_NOT_SET, missing
            assert _code(ctx.align, solve=binding.SOLVE_KABSCH, max_iterations=2) == 0, missing
            ctx.nn(binding.NN_GRID, fetch=False)
            assert _code(ctx.reduce_colored) == binding.E_NOT_SET, missing
        install()
        assert _code(ctx.align, solve=P2L, max_iterations=2) == 0
        assert _code(ctx.align, solve=P2L, nn_mode=binding.NN_MAP) == binding.E_ARG
        ctx.set_robust(binding.ROBUST_HUBER, 1.0, binding.SCALE_MEDIAN, 1.0)
        assert _code(ctx.align, solve=P2L, max_iterations=2) == binding.E_ARG
        assert _code(ctx.align, solve=binding.SOLVE_KABSCH, max_iterations=2) == 0
        ctx.set_robust(None)
        assert _code(ctx.align_query_sharded, solve=P2L) == binding.E_ARG
        assert _code(ctx.align_to_map, solve=P2L) == binding.E_ARG
        assert _code(ctx.align_to_map_dense, solve=P2L) == binding.E_ARG
        assert _code(ctx.align, solve=P2L, max_iterations=2) == 0
    finally:
        ctx.set_robust(None)
        ctx.set_colored(False)


def test_lifetime(ctx):
    import torch

    rng = np.random.default_rng(3)
    p = synth.kinect_pair(rows=60, cols=80, seed=5)
    src, tgt = p["source"], p["target"]
    ns, nt = src.shape[1], tgt.shape[1]
    depth = p["depth_src"]
    sdev = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    tdev = torch.from_numpy(np.ascontiguousarray(tgt)).cuda()
    gray = (rng.integers(0, 2, depth.shape) * 255).astype(np.uint8)
    sc, tc = rng.uniform(0, 1, ns).astype(np.float32), rng.uniform(0, 1, nt).astype(np.float32)

    def install():
        ctx.set_target(tgt)
        ctx.set_target_normals(_unit(rng, nt))
        ctx.set_target_colors(tc)
        ctx.estimate_target_color_gradients(0.05, 4, keep_sums=True)
        ctx.set_source(src)
        ctx.set_source_colors(sc)

    def fast_cloud(which):
        ctx.detect_fast(gray, threshold=20)
        ctx.detected_to_cloud(depth, which=which)

    def map_target(lookup):
        ctx.map_reset()
        ctx.map_update_points(binding.MAP_ADD_CLOUD, tgt, binding.MAP_DELTA_CONFIDENCE)
        ctx.map_lookup_to_target() if lookup else ctx.map_list_to_target(binding.MAP_POINTS)

    drops_source = {
        "set_source": lambda: ctx.set_source(src),
        "set_source_device": lambda: ctx.set_source_device(sdev[0].data_ptr(), sdev[1].data_ptr(), sdev[2].data_ptr(), ns),
        "backproject": lambda: ctx.backproject(depth, which=0),
        "backproject_filtered": lambda: ctx.backproject_filtered(depth, which=0),
        "detected_to_cloud": lambda: fast_cloud(0),
        "voxel_downsample": lambda: ctx.voxel_downsample(0, 0.05),
        "remove_outliers": lambda: ctx.remove_outliers(0, kind=binding.FILTER_RADIUS, radius=0.1, min_neighbors=2),
    }
    drops_target = {
        "set_target": lambda: ctx.set_target(tgt),
        "set_target_device": lambda: ctx.set_target_device(tdev[0].data_ptr(), tdev[1].data_ptr(), tdev[2].data_ptr(), nt),
        "backproject": lambda: ctx.backproject(depth, which=1),
        "backproject_filtered": lambda: ctx.backproject_filtered(depth, which=1),
        "backproject_with_normals": lambda: ctx.backproject_with_normals(depth),
        "detected_to_cloud": lambda: fast_cloud(1),
        "voxel_downsample": lambda: ctx.voxel_downsample(1, 0.05),
        "remove_outliers": lambda: ctx.remove_outliers(1, kind=binding.FILTER_RADIUS, radius=0.1, min_neighbors=2),
        "map_list_to_target": lambda: map_target(False),
        "map_lookup_to_target": lambda: map_target(True),
        "tsdf_surface_to_target": lambda: tsdf_cases.hand_over(ctx, raycast=False),
        "tsdf_raycast_to_target": lambda: tsdf_cases.hand_over(ctx, raycast=True),
    }
    for name, act in drops_source.items():
        install()
        act()
        assert _code(ctx.get_source_colors) == binding.E_NOT_SET, name
        assert ctx.get_target_colors().tobytes() == tc.tobytes(), name
        assert ctx.get_target_color_gradients().shape == (3, nt), name
    for name, act in drops_target.items():
        install()
        act()
        assert _code(ctx.get_target_colors) == binding.E_NOT_SET, name
        assert _code(ctx.get_target_color_gradients) == binding.E_NOT_SET, name
        assert _code(ctx.color_gradient_sums) == binding.E_NOT_SET, name
        assert ctx.get_source_colors().tobytes() == sc.tobytes(), name
    # a TSDF volume with ICPK_TSDF_COLOR hands its own intensities over with the points: the new target has colours
    # (the volume's, one per point), and neither the old target's gradients nor their sums
    for raycast in (False, True):
        install()
        n = tsdf_cases.hand_over(ctx, raycast=raycast, color=True)
        got = ctx.get_target_colors()
        assert got.shape == (n,) and got.tobytes() != tc[:n].tobytes() and np.all(np.abs(got - 0.5) < 1e-6), raycast
        assert _code(ctx.get_target_color_gradients) == binding.E_NOT_SET, raycast
        assert _code(ctx.color_gradient_sums) == binding.E_NOT_SET, raycast
        assert ctx.get_target_normals().shape == (3, n), raycast
        assert ctx.get_source_colors().tobytes() == sc.tobytes(), raycast
    ctx.tsdf_release()
    install()
    ctx.backproject_pair(depth, p["depth_tgt"])
    assert _code(ctx.get_source_colors) == binding.E_NOT_SET and _code(ctx.get_target_colors) == binding.E_NOT_SET
    assert _code(ctx.get_target_color_gradients) == binding.E_NOT_SET
    ctx.map_release()
    # what keeps them: moving, resetting and committing the source, the loop, statistics-only filters; new target
    # intensities drop the gradients only
    install()
    g = ctx.get_target_color_gradients()
    ctx.transform_source(synth.rot_xyz_deg(1, 2, 3).astype(np.float32), np.float32([0.01, 0, 0]))
    ctx.commit_source()
    ctx.reset_source()
    ctx.align(solve=binding.SOLVE_KABSCH, max_iterations=2)
    ctx.remove_outliers(0, kind=binding.FILTER_RADIUS, radius=0.1, min_neighbors=2, stats_only=True)
    ctx.remove_outliers(1, kind=binding.FILTER_RADIUS, radius=0.1, min_neighbors=2, stats_only=True)
    assert ctx.get_source_colors().tobytes() == sc.tobytes() and ctx.get_target_colors().tobytes() == tc.tobytes()
    assert ctx.get_target_color_gradients().tobytes() == g.tobytes()
    assert ctx.color_gradient_sums().shape == (nt, 10)
    ctx.set_target_colors(tc)
    assert _code(ctx.get_target_color_gradients) == binding.E_NOT_SET
    assert ctx.get_source_colors().tobytes() == sc.tobytes()


def test_transform_target_rotates_the_gradients(ctx):
    p = cm.wall_pair(rows=20, cols=30, relief=0.003)
    ctx.set_target(p["target"])
    ctx.set_target_normals(p["target_normals"])
    ctx.set_target_colors(p["target_intensity"])
    ctx.estimate_target_color_gradients(cm.WALL_RADIUS, cm.WALL_MIN_NB, keep_sums=True)
    g = ctx.get_target_color_gradients()
    assert (g != 0).any(0).mean() > 0.9
    R, t = synth.rot_xyz_deg(10, -20, 30).astype(np.float32), np.float32([0.1, 0.2, -0.3])
    ctx.transform_target(R, t)
    moved = ctx.get_target_color_gradients()
    assert ctx.get_target_colors().tobytes() == p["target_intensity"].tobytes()
    assert _code(ctx.color_gradient_sums) == binding.E_NOT_SET  # (taken along the old axes)
    # exactly what the call does to normals: the gradients given as normals and moved the same way
    ctx.set_target(p["target"])
    ctx.set_target_normals(g)
    ctx.transform_target(R, t)
    assert moved.tobytes() == ctx.get_target_normals().tobytes()
    assert np.abs(moved.astype(np.float64) - R.astype(np.float64) @ g.astype(np.float64)).max() < 1e-5 * np.abs(g).max()
