"""Every linearised step on the device held against central differences of the cost it claims to minimise.

tests/test_gauss_newton_host.py holds the numpy models and the rule headers, per pair; here the DEVICE sums of the seven
flavours -- icpk_reduce_p2l (K5), icpk_reduce_plane_to_plane (K14), icpk_reduce_colored (K17), icpk_projective_reduce
(K25, and K28 through ICPK_VIEW_FRAME), icpk_projective_reduce_colored (K26), icpk_sdf_reduce (K29) -- are compared
with tests/gauss_newton_reference.py directly: no model in between.  The reference is handed what the device holds
(associations, view planes, gradients, tsdf planes, all read back from the context), applies the flavour's acceptance
test itself, and sums J^T J and J^T r of central differences in np.longdouble.  Then one iteration of every loop must
land on [exp([omega]x) | t] E_0 with x = -H_ref^-1 b_ref by the reference's own elimination: that pins the solve,
Rodrigues and the order of composition on the device path.

Tolerances: the per-pair bounds of the reference module (the central difference's own error, the rule's float32
roundings propagated linearly, the float64 arithmetic of the terms) summed over the pairs, plus the float64 tree,
n 2^-53 sum |term|.  For a pose, |H^-1| (|db| + |dH| |x|) with those bounds, the Cholesky solve's 57 cond 2^-52 |x|, and
for the cloud flavours one float32 ulp per entry, because their motion is applied and recorded in float.  Nothing is
tuned to an observed error; every test prints error / bound, and repeats the comparison against deliberately wrong
references (the cross product reversed, lg and lc swapped, R_acc left off, r negated, dT composed on the right), from
each of which the device must lie at least FAR bounds away.

Shapes: clouds of 257 and 1000 points (one and four reduction blocks, a ragged last block); images 7 x 9, 17 x 19 and
60 x 80 (less than a wave, two blocks, nineteen)."""
import numpy as np
import pytest

import frame_view_cases as fc
import gauss_newton_reference as gn
import projective_cases as pc
import projective_color_cases as qc
import sdf_track_cases as sc
from icp_slam_prototype_amd import binding, depth

pytestmark = pytest.mark.gpu

FAR = 100.0
MAX_DIST = np.float32(0.75)
EPSILON = np.float32(1e-3)
LAMBDA = np.float32(0.968)
GRADIENT_RADIUS, GRADIENT_MIN_NB = 0.25, 4
P2L, P2P = binding.SOLVE_POINT_TO_PLANE, binding.SOLVE_PLANE_TO_PLANE


@pytest.fixture(scope="module")
def ctx():
    with binding.Context(0) as c:
        yield c


# ---- sums and poses against a reference with bounds -------------------------------------------------------------------
def total(ref, rows):
    """a per-pair reference summed: dict(H (6, 6), b (6,), dH, db), the float64 tree over `rows` rows included"""
    H, b = ref["H"].sum(0), ref["b"].sum(0)
    return dict(H=H, b=b, dH=ref["dH"].sum(0) + gn.tree_error(rows, np.abs(ref["H"]).sum(0)),
                db=ref["db"].sum(0) + gn.tree_error(rows, np.abs(ref["b"]).sum(0)))


def hold_sums(what, sums, ref, wrongs):
    H, b, _ = gn.unpack(sums)
    wH, wb = gn.worst(H, ref["H"], ref["dH"]), gn.worst(b, ref["b"], ref["db"])
    far = {k: max(gn.worst(H, w["H"], ref["dH"]), gn.worst(b, w["b"], ref["db"])) for k, w in wrongs.items()}
    print(f"{what}: worst error / bound H {wH:.3g}, b {wb:.3g}; relative bound H {float(np.abs(ref['dH']).max() / np.abs(ref['H']).max()):.3g}"
          f", b {float(np.abs(ref['db']).max() / np.abs(ref['b']).max()):.3g}; wrong references at "
          + ", ".join(f"{k} {v:.3g}" for k, v in far.items()) + " bounds")
    assert wH <= 1 and wb <= 1, (what, wH, wb)
    for k, v in far.items():
        assert v >= FAR, (what, k, v)


def hold_distance_sum(what, got, dists, rows):
    want = float(np.sum(np.asarray(dists, np.float32).astype(np.float64)))
    assert abs(got - want) <= rows * 2.0 ** -53 * want, (what, got, want)


def step_bound(ref):
    """(x, dx (6,)): the reference's motion and the bound on the device's, entry by entry: |H^-1| (db + dH |x|) / (1 - rho),
    rho = | |H^-1| dH |, plus the Cholesky solve's 57 cond 2^-52 |x| (tests/test_gauss_newton_host.py derives it)"""
    x = gn.step(ref["H"], ref["b"])
    Hi = np.abs(gn.inverse6(ref["H"]))
    rho = float(np.linalg.norm(np.asarray(Hi @ ref["dH"], np.float64), 2))
    assert rho < 0.5
    H64 = np.asarray(ref["H"], np.float64)
    cond = np.linalg.norm(H64, 2) * np.linalg.norm(np.linalg.inv(H64), 2)
    return x, Hi @ (ref["db"] + ref["dH"] @ np.abs(x)) / (1 - rho) + 57 * cond * 2.0 ** -52 * np.sqrt(x @ x)


def hold_pose(what, pose, E0, ref, wrongs, float_ulp=False):
    """pose (4, 4) of one iteration from E0 = [R0 | t0] against [exp | t] E0 of the reference's step.  The exponential map
    does not expand, so an entry of exp R0 moves by at most |d omega| and one of exp t0 + t by |d omega| |t0| + dt; eight
    float64 roundings for the composition.  wrongs: name -> (wrong reference or None for the right one, the `wrong` of
    stepped_pose)."""
    x, dx = step_bound(ref)
    want = gn.stepped_pose(x, E0)
    dw = np.sqrt((dx[:3] ** 2).sum())
    t0 = np.sqrt((gn.ld(E0)[:3, 3] ** 2).sum())
    bound = np.concatenate([np.full((3, 3), dw), (dw * t0 + dx[3:])[:, None]], axis=1) + 8 * gn.U64 * np.abs(want[:3])
    if float_ulp:
        bound = bound + 2.0 ** -23 * np.abs(want[:3])
    w = gn.worst(pose[:3], want[:3], bound)
    far = {}
    for k, (wr, how) in wrongs.items():
        far[k] = gn.worst(pose[:3], gn.stepped_pose(gn.step(wr["H"], wr["b"]) if wr is not None else x, E0, how)[:3], bound)
    print(f"{what}: |x| {float(np.sqrt(x @ x)):.3g}, pose worst error / bound {w:.3g}, bound {float(bound.max()):.3g}; wrong references at "
          + ", ".join(f"{k} {v:.3g}" for k, v in far.items()) + " bounds")
    assert np.array_equal(np.asarray(pose)[3], [0, 0, 0, 1])
    assert w <= 1, (what, w)
    for k, v in far.items():
        assert v >= FAR, (what, k, v)


# ---- clouds (K5, K14, K17) --------------------------------------------------------------------------------------------
def cloud(n, seed=11):
    """n target points: a 1.2 m box of random points and six isolated ones a metre apart (no neighbour within the gradient
    radius: the zero gradient); the source is a noisy copy with four points moved beyond max_dist; random unit normals on
    both sides with a few zero normals, one source normal of length 1.5 and one of 0.5, set from the host"""
    rng = np.random.default_rng(seed + n)
    F = np.float32
    unit = lambda v: (v / np.linalg.norm(v, axis=0)).astype(F)
    tgt = (rng.uniform(-0.6, 0.6, (3, n)) + [[0], [0], [2]]).astype(F)
    tgt[:, :6] = np.array([[3.0 + k, 3.0, 2.0] for k in range(6)], F).T
    src = (tgt + rng.normal(0, 0.01, (3, n))).astype(F)
    src[2, 20:24] += F(5)
    tnrm, snrm = unit(rng.normal(size=(3, n))), unit(rng.normal(size=(3, n)))
    tnrm[:, 30:35] = 0
    snrm[:, 40:43] = 0
    snrm[:, 7] *= F(1.5)
    snrm[:, 8] *= F(0.5)
    return dict(src=src, tgt=tgt, tnrm=tnrm, snrm=snrm, tcol=rng.random(n).astype(F), scol=rng.random(n).astype(F))


def rotations():
    general = np.asarray(gn.exp_so3([0.3, -0.5, 0.2]), np.float64).astype(np.float32)
    return {"identity": None, "permutation": np.float32([[0, -1, 0], [0, 0, 1], [-1, 0, 0]]), "general": general}


def upload(ctx, c):
    ctx.set_target(c["tgt"])
    ctx.set_source(c["src"])
    ctx.set_target_normals(c["tnrm"])
    ctx.set_source_normals(c["snrm"])
    ctx.set_target_colors(c["tcol"])
    ctx.set_source_colors(c["scol"])
    ctx.estimate_target_color_gradients(GRADIENT_RADIUS, GRADIENT_MIN_NB)
    ctx.set_plane_to_plane(float(EPSILON))
    ctx.set_colored(False, float(LAMBDA))
    return ctx.get_target_color_gradients()


def cloud_reference(c, grad, idx, dist, flavour, R_acc=None, wrong=None):
    """the flavour's acceptance test applied here, then the reference over the accepted pairs: (per-pair reference, mask)"""
    near = dist < MAX_DIST
    j = np.where(near, idx, 0)
    p, q, n = c["src"], c["tgt"][:, j], c["tnrm"][:, j]
    if flavour == "gicp":
        form = "cost" if R_acc is None or np.array_equal(np.abs(R_acc).sum(0), [1, 1, 1]) else "rule"
        _, S = gn.gicp_metric(c["snrm"], n, R_acc, EPSILON, "rule")
        det = np.linalg.det(np.asarray(S, np.float64))
        acc = near & np.isfinite(det) & (det > 0)
        return gn.gicp_pairs(p[:, acc], q[:, acc], c["snrm"][:, acc], n[:, acc], R_acc, EPSILON, form, wrong), acc
    acc = near & (n != 0).any(0)
    if flavour == "p2l":
        return gn.p2l_pairs(p[:, acc], q[:, acc], n[:, acc], wrong=wrong), acc
    return gn.colored_pairs(p[:, acc], q[:, acc], n[:, acc], grad[:, j][:, acc], c["tcol"][j][acc], c["scol"][acc], LAMBDA, wrong=wrong), acc


CLOUD_FLAVOURS = [("p2l", None), ("colored", None), ("gicp", "identity"), ("gicp", "permutation"), ("gicp", "general")]
CLOUD_WRONGS = {"p2l": ("cross", "negate"), "colored": ("cross", "swap", "negate"), "gicp": ("cross", "negate")}


@pytest.mark.parametrize("n", (257, 1000))
@pytest.mark.parametrize("flavour,rotation", CLOUD_FLAVOURS)
def test_cloud_sums_are_the_gauss_newton_system(ctx, n, flavour, rotation):
    c = cloud(n)
    grad = upload(ctx, c)
    ctx.nn(binding.NN_EXACT, fetch=False)
    idx, dist = ctx.get_associations()
    R = rotations()[rotation] if rotation else None
    if flavour == "p2l":
        sums, count = ctx.reduce_p2l(float(MAX_DIST))
    elif flavour == "colored":
        sums, count = ctx.reduce_colored(float(MAX_DIST))
    else:
        sums, count = ctx.reduce_plane_to_plane(float(MAX_DIST), R)
    ref, acc = cloud_reference(c, grad, idx, dist, flavour, R)
    assert count == int(acc.sum())  # as integers
    near = dist < MAX_DIST
    assert 0 < (~near).sum() <= 8 and (near & ~acc).any()  # pairs beyond max_dist, and pairs the flavour's own test rejects
    if flavour == "colored":
        g = grad[:, idx[acc]]
        assert (g == 0).all(0).any() and (g != 0).any(0).any()  # pairs with the zero gradient among the others
    if flavour == "gicp":
        assert not acc[7] and acc[8]  # the source normal of length 1.5 makes S indefinite; the one of 0.5 is accepted
    names = CLOUD_WRONGS[flavour] + (("no_R",) if rotation in ("permutation", "general") else ())
    wrongs = {w: total(cloud_reference(c, grad, idx, dist, flavour, R, w)[0], n) for w in names}
    hold_sums(f"{flavour}{' R_acc ' + rotation if rotation else ''}, n {n}", sums, total(ref, n), wrongs)
    hold_distance_sum(flavour, sums[27], dist[acc], n)


@pytest.mark.parametrize("host_loop", (0, 1))
@pytest.mark.parametrize("flavour", ("p2l", "colored", "gicp"))
def test_one_cloud_iteration_is_the_gauss_newton_step(ctx, flavour, host_loop):
    n = 257
    c = cloud(n)
    grad = upload(ctx, c)
    ctx.nn(binding.NN_EXACT, fetch=False)
    idx, dist = ctx.get_associations()
    ctx.set_colored(flavour == "colored", float(LAMBDA))
    try:
        T, st, rc = ctx.align(max_iterations=1, fixed_iterations=1, nn_mode=binding.NN_EXACT, max_nn_dist=float(MAX_DIST),
                              solve=P2P if flavour == "gicp" else P2L, host_loop=host_loop)
    finally:
        ctx.set_colored(False, float(LAMBDA))
    assert rc == binding.OK and st.iterations == 1
    ref = total(cloud_reference(c, grad, idx, dist, flavour)[0], n)
    wrongs = {w: (total(cloud_reference(c, grad, idx, dist, flavour, None, w)[0], n), None) for w in ("cross", "negate")}
    hold_pose(f"{flavour}, host_loop {host_loop}", T.astype(np.float64), np.eye(4), ref, wrongs, float_ulp=True)


# ---- images (K25, K26, K28, K29) --------------------------------------------------------------------------------------
IMAGE_CASES = [("K25", n) for n in ("7x9", "17x19", "room_l1")] + [("K26", n) for n in ("7x9", "17x19", "room_l1")] \
    + [("K28", 1), ("K28", 2), ("K28 coloured", 1)] + [("K29", n) for n in ("7x9", "17x19", "room_l1", "shifted")]
IMAGE_WRONGS = {"K25": ("cross", "negate"), "K26": ("cross", "swap", "negate"), "K28": ("cross", "negate"),
                "K28 coloured": ("cross", "swap", "negate"), "K29": ("cross", "negate")}
COLOR = dict(lambda_geometric=float(LAMBDA))
# K29's step is held on the 60 x 80 images only.  Its 7 x 9 and 17 x 19 cases accept 42 and 158 pixels; their 6 x 6 has a
# condition number of 3.4e3 and 1.6e4, and the float32 bound of the sums (2e-5 .. 6e-5 relative: the normal is a quotient
# of float32 differences) grows through |H^-1| to a pose bound of 4e-3 and 0.16, next to a motion of 0.2 and 0.8: that
# bound separates nothing.  These figures come from the reference and its bounds alone; the sums of both cases are held.
NO_STEP = {("K29", "7x9"), ("K29", "17x19")}


@pytest.fixture
def viewed(ctx):
    yield ctx
    binding.projective_set_view(ctx, binding.VIEW_RAYCAST)


def raycast_planes(c):
    m = c.tsdf_get_raycast()
    return np.concatenate([m["points"], m["normals"], m["depth"][None], m["intensity"][None]])


def image_case(c, kind, name):
    """The case set up on the context, one evaluation of the device's sums at the case's estimate, and what the reference
    needs, READ BACK from the context.  Returns dict(E, params, sums, count, rows, dists, args, kw, align)."""
    if kind in ("K25", "K26"):
        cases = pc if kind == "K25" else qc
        k = cases.case(name)
        p = cases.device_setup(c, name, depth, binding)
        E, level, fx, cx = k["estimate"], k["level"], k["fx"], k["cx"]
        planes = raycast_planes(c)
        grad = binding.get_raycast_color_gradients(c) if kind == "K26" else None
    elif kind.startswith("K28"):
        level, colored = name, kind.endswith("coloured")
        k = fc.case("room_color")
        fc.device_setup(c, "room_color", depth)
        binding.frame_view_build(c, k["pose"], fx=k["fx"], cx=k["cx"])
        if colored:
            binding.frame_view_color_gradients(c, level, fc.GRADIENT_RADIUS * 2 ** level)
        f = fc.next_frame()
        depth.build_pyramid(c, f["depth"], depth.pyramid_params(levels=3), intensity=f["intensity"])
        binding.projective_set_view(c, binding.VIEW_FRAME, level)
        p = binding.default_projective_params(level=level, fx=k["fx"], cx=k["cx"])
        E, fx, cx = k["pose"], k["fx"], k["cx"]
        planes = binding.frame_view(c, level)
        grad = binding.frame_view_get_color_gradients(c, level) if colored else None
    else:
        k = sc.case(name)
        p = sc.device_setup(c, name, depth, binding)
        E, level, fx, cx = k["estimate"], k["level"], k["fx"], k["cx"]
    scale = np.float32(2 ** level)
    img, fx_s, cx_s = depth.pyramid_level(c, level), np.float32(fx) / scale, np.float32(cx) / scale
    if kind == "K29":
        cell, value = binding.sdf_associate(c, E, p)
        sums, count = binding.sdf_reduce(c, E, p)
        f, _, _ = c.tsdf_get()
        tp = binding.tsdf_get_params(c)[0]
        field = gn.Trilinear(f, np.array(tp.origin, np.float32), tp.voxel, tp.trunc)
        return dict(E=E, params=p, sums=sums, count=count, rows=img.size, accepted=int((cell >= 0).sum()),
                    dists=np.abs(value[cell >= 0]), reference=lambda wrong=None: gn.sdf_image(img, fx_s, cx_s, E, cell, field, wrong),
                    align=lambda q: binding.align_sdf(c, E, q))
    pixel, dist = binding.projective_associate(c, E, p)
    if grad is None:
        sums, count = binding.projective_reduce(c, E, p)
        color, align = None, lambda q: binding.align_projective(c, E, q)
    else:
        sums, count = binding.projective_reduce_colored(c, E, p, color=COLOR)
        color = dict(level_intensity=binding.pyramid_intensity(c, level), gradient=grad, lambda_geometric=LAMBDA)
        align = lambda q: binding.align_projective_colored(c, E, q, color=COLOR)
        g = grad.reshape(3, -1)[:, pixel[pixel >= 0]]
        assert (g != 0).any()
    return dict(E=E, params=p, sums=sums, count=count, rows=img.size, accepted=int((pixel >= 0).sum()), dists=dist[pixel >= 0],
                reference=lambda wrong=None: gn.projective_pixels(img, fx_s, cx_s, E, pixel, planes, color, wrong), align=align)


@pytest.mark.parametrize("kind,name", IMAGE_CASES)
def test_image_sums_and_one_iteration_are_the_gauss_newton_system_and_step(viewed, kind, name):
    """K29: the reference's row is the numeric derivative of D(exp(x) p) divided by its translational length kappa -- the
    rule normalises the gradient (tests/test_gauss_newton_host.py states the deviation and holds it per pixel); a pixel
    keeps the cell the device reports, whose own polynomial the reference evaluates."""
    k = image_case(viewed, kind, name)
    what = f"{kind} {name}"
    assert k["count"] == k["accepted"] >= 6  # as integers: the association is the device's own
    ref = total(k["reference"](), k["rows"])
    wrongs = {w: total(k["reference"](w), k["rows"]) for w in IMAGE_WRONGS[kind]}
    hold_sums(what, k["sums"], ref, wrongs)
    hold_distance_sum(what, k["sums"][27], k["dists"], k["rows"])
    if (kind, name) in NO_STEP:
        return
    # one iteration from the same estimate
    q = k["params"]
    q.max_iterations = 1
    pose, res = k["align"](q)
    assert res.status == binding.OK and res.iterations == 1 and res.count == k["count"]
    step_wrongs = {w: (r, None) for w, r in wrongs.items() if w in ("cross", "negate")}
    step_wrongs["right"] = (None, "right")
    hold_pose(what, pose, k["E"], ref, step_wrongs)
