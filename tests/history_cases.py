"""The history matrix (tests/test_history_host.py, tests/test_gpu_history.py): for fixed inputs and fixed settings every
public result of a context is the same bytes whatever the context did before.

A PROBE is a function probe(ctx, scene) -> dict[str, Blob]: it installs everything it needs through public calls --
every persistent setting included, each set to the probe's own value (`settings`) -- and returns every output of one
feature as raw bytes.  A HISTORY is a function history(ctx) that leaves the context in some state and asserts nothing.
The GPU test runs a history, then every probe on the probe scene, and compares each with the bytes a fresh context
gave.  No GPU is touched when this module is imported.

The scenes (seeded numpy through `synth`, nothing read from disk).  The sizes come from the constants of the code:
NN_TILE = 1024 (csrc/icpk_internal.h: the pad of every cloud buffer and the tile of the NN kernels), COMPACT_BLOCK = 256
(the workgroup size with which the cloud compactions of K11 and K13 instantiate csrc/block_scan.h: block_total<256> /
block_excl_scan<256> in kernels_voxel.hip and kernels_filter.hip; the host test reads both figures from the sources),
the wave of 64 lanes, SCORE_MAX_POSES = 4096 (include/icpk.h).

  P  the probe scene: synth.kinect_pair at 40 x 60, valid 0.7, seed 11: 1642 source and 1697 target points.  Above
     NN_TILE and below two (two tiles, the second partly filled); seven workgroups of COMPACT_BLOCK in the cloud
     compactions, the last partly filled, so their per-block sums are scanned across blocks.  Small enough for the
     numpy models (tests/test_history_host.py states what each model finds on it).  Offset (5, 5, 5), the start of
     the reference's camera: inside the certainty map's [0, 10) m.
  Q  the large and different scene: 60 x 80, seed 5, 3394 / 3347 points (2 x P: four tiles, every buffer P uses is
     grown past P's padded size and P then sits in a large allocation with a finite stale tail; no larger, because
     the file's time does not buy more with a larger Q: DESIGN.md section 8), scaled by 1.7 and offset
     (6.5, 3.0, 1.0): another bounding box, another cell size, another cell count and another Morton box than P's.
  S  the tiny scene: 37 points a side (6 x 8 pixels, 11 of them blanked): below one wave (64), one tile and one
     compaction block; gives the shrink-then-grow transitions.

Early-path histories (EARLY): each ends on a path include/icpk.h defines with a return code; none is a fault.  The
non-finite cloud of `early_non_finite` goes only through the calls whose header paragraph states a rule for non-finite
points: K12 (normals), K13 (outlier filters), K16 (FPFH, matching) and K17 (colour gradients).  Left out of that one
history because the header gives no rule for non-finite points there: the NN sweeps and every alignment (include/icpk.h
line 20: clouds are expected to be finite), K11 voxel downsampling's centroid, K14's reduction, the TSDF, the front
end and the batches.

icpk_score_poses refuses more than SCORE_MAX_POSES poses per call (ICPK_E_ARG), so the score probe sends exactly
SCORE_MAX_POSES, the refusal is part of `early_refusals`, and the chunking beyond SCORE_MAX_POSES is crossed by the
FPFH probe's register_global (more valid hypotheses than one chunk).

Shared-state histories (SHARED): `shared_aux_index` leaves the index that the source normals (K14), the source's
descriptors (K16) and the filter of the working source (K13) build in turn as the last of them built it on Q.

COVERAGE maps every public name of binding.Context to the probes and histories that call it, or to EXEMPT with a
reason; tests/test_history_host.py holds it against the class."""
import functools

import numpy as np

from icp_slam_prototype_amd import binding, synth

NN_TILE = 1024     # csrc/icpk_internal.h
COMPACT_BLOCK = 256  # kernels_voxel.hip, kernels_filter.hip: block_total<256> / block_excl_scan<256>
WAVE = 64

B = binding
P2L, GICP = B.SOLVE_POINT_TO_PLANE, B.SOLVE_PLANE_TO_PLANE


class Blob(bytes):
    """raw bytes of one output, with the dtype and shape they were read from (for the failure message only)"""
    dtype = None
    shape = None


def blob(x):
    if isinstance(x, (bytes, bytearray)):
        return Blob(x)
    a = np.ascontiguousarray(x)
    out = Blob(a.tobytes())
    out.dtype, out.shape = a.dtype, a.shape
    return out


def first_difference(a, b):
    """where two blobs differ, in words: the first differing element if they are arrays of one dtype and shape"""
    if len(a) != len(b):
        return f"{len(a)} bytes against {len(b)} (shapes {getattr(a, 'shape', None)} / {getattr(b, 'shape', None)})"
    dt = getattr(a, "dtype", None)
    if dt is None or dt != getattr(b, "dtype", None) or dt.itemsize == 0:
        k = next(i for i in range(len(a)) if a[i] != b[i])
        return f"first differing byte {k}"
    x, y = np.frombuffer(a, dt), np.frombuffer(b, dt)
    raw = dt.itemsize
    d = np.flatnonzero((np.frombuffer(a, np.uint8).reshape(-1, raw) != np.frombuffer(b, np.uint8).reshape(-1, raw)).any(1))
    k = int(d[0])
    return f"{d.size} of {x.size} {dt} elements differ (shape {a.shape}), first at flat index {k}: {x[k]!r} against {y[k]!r}"


# ------------------------------------------------------------------------------------------------------ scenes --
def _intensity(rows, cols, P, fx, cx, cell):
    bgr = synth.render_room_color(rows, cols, P[:3, :3], P[:3, 3], fx, cx, cell=cell)
    return bgr, (bgr.astype(np.float64).sum(-1) / 765.0).astype(np.float32)  # (icpk_intensity_from_bgr's formula)


def _scene(name, rows, cols, valid, seed, fx, cx, offset, scale, blank=0, cell=0.9):
    p = synth.kinect_pair(rows=rows, cols=cols, valid=valid, seed=seed, fx=fx, cx=cx, world_offset=False)
    ds, dt = p["depth_src"].copy(), p["depth_tgt"].copy()
    rng = np.random.default_rng(seed + 100)
    for d in (ds, dt):  # blank `blank` valid pixels (S: down to 37 points)
        r, c = np.nonzero(d)
        kill = rng.choice(r.size, blank, replace=False) if blank else []
        d[r[kill], c[kill]] = 0
    pose_t = np.eye(4)
    pose_s = np.eye(4)
    pose_s[:3, :3], pose_s[:3, 3] = p["R_true"], p["t_true"]
    cam_s, cam_t = synth.backproject(ds, None, fx, cx), synth.backproject(dt, None, fx, cx)
    off = np.asarray(offset, np.float32)
    sc = np.float32(scale)
    src = (cam_s * sc + off[:, None]).astype(np.float32)
    tgt = (cam_t * sc + off[:, None]).astype(np.float32)
    bgr_s, img_s = _intensity(rows, cols, pose_s, fx, cx, cell)
    bgr_t, img_t = _intensity(rows, cols, pose_t, fx, cx, cell)
    nrm = rng.normal(size=(3, tgt.shape[1]))
    nrm = (nrm / np.linalg.norm(nrm, axis=0)).astype(np.float32)
    snrm = rng.normal(size=(3, src.shape[1]))
    snrm = (snrm / np.linalg.norm(snrm, axis=0)).astype(np.float32)
    # the source cloud in the TSDF's world (camera-to-world pose of the source frame, no offset, no scale)
    world_s = (pose_s[:3, :3] @ cam_s.astype(np.float64) + pose_s[:3, 3:4]).astype(np.float32)
    s = dict(name=name, rows=rows, cols=cols, fx=float(fx), cx=float(cx), scale=float(scale), offset=off,
             source=src, target=tgt, depth_src=ds, depth_tgt=dt, pose_src=pose_s, pose_tgt=pose_t,
             R=np.asarray(p["R_true"], np.float32), t=(np.asarray(p["t_true"], np.float32) + off).astype(np.float32),
             source_intensity=np.ascontiguousarray(img_s[ds != 0]), target_intensity=np.ascontiguousarray(img_t[dt != 0]),
             image_src=img_s, image_tgt=img_t, bgr=bgr_t, target_normals=nrm, source_normals=snrm, source_world=world_s,
             viewpoint=off.copy(), seed=seed)
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return s


SCENE_ARGS = {
    "P": dict(rows=40, cols=60, valid=0.7, seed=11, fx=44.0, cx=29.5, offset=(5.0, 5.0, 5.0), scale=1.0),
    "Q": dict(rows=60, cols=80, valid=0.7, seed=5, fx=58.0, cx=39.5, offset=(6.5, 3.0, 1.0), scale=1.7),
    "S": dict(rows=6, cols=8, valid=1.0, seed=3, fx=6.0, cx=3.5, offset=(5.0, 5.0, 5.0), scale=1.0, blank=11),
}


def build_scene(name):
    """a scene built afresh (the host test compares two builds)"""
    return _scene(name, **SCENE_ARGS[name])


@functools.lru_cache(maxsize=None)
def scene(name):
    """the scene, built once per process and read-only"""
    return build_scene(name)


# figures every probe derives from the scene (metres scale with the scene)
def radius(s):
    return 0.25 * s["scale"]           # K12 / K14 / K17 neighbourhoods: some tens of neighbours on P


def fpfh_radius(s):
    return 0.45 * s["scale"]


def max_dist(s):
    return 0.12 * s["scale"]   # cuts some pairs of P off, keeps most


def leaf(s):
    return 0.15 * s["scale"]


TSDF_VOLUME = dict(dims=(33, 31, 29), voxel=0.125, origin=(-2.3, -1.9, 0.4), trunc=0.375)  # odd dims: chunks end mid-row
RAY_VIEW = dict(z_near=0.25, z_far=6.0, step=0.125, min_weight=1)
FAST_THRESHOLD = 20
MOVE_R = synth.rot_xyz_deg(0.4, -0.3, 0.5).astype(np.float32)
MOVE_T = np.float32([0.006, -0.004, 0.003])


# ------------------------------------------------------------------------------------------------------ probes --
def settings(ctx):
    """every persistent setting at the probes' value (settings persist by design: leaking them is not what is tested)"""
    ctx.set_robust(None)
    ctx.set_colored(False, 0.968)
    ctx.set_plane_to_plane(1e-3)
    ctx.set_subsample(0, 0)


def clouds(ctx, s):
    ctx.set_target(s["target"])
    ctx.set_source(s["source"])


def _stats(out, key, st):
    out[key + ".stats"] = blob(np.array([st.iterations, st.status, st.final_pairs, st.nn_launches, st.nn_timed_launches],
                                        np.int32))
    out[key + ".mse"] = blob(np.float32(st.final_mse))


def _trace(out, key, tr):
    out[key + ".trace_n"] = blob(np.int32(len(tr)))
    if tr:
        out[key + ".trace_R"] = blob(np.stack([x["R"] for x in tr]))
        out[key + ".trace_t"] = blob(np.stack([x["t"] for x in tr]))
        out[key + ".trace_pairs"] = blob(np.array([x["n_pairs"] for x in tr], np.int32))
        out[key + ".trace_mse"] = blob(np.array([x["mse"] for x in tr], np.float32))


def _aligned(ctx, out, key, res, robust=False):
    """everything an alignment exposes"""
    T, st, rc = res
    out[key + ".T"] = blob(T)
    out[key + ".rc"] = blob(np.int32(rc))
    _stats(out, key, st)
    idx, dist = ctx.get_associations()
    out[key + ".idx"], out[key + ".dist"] = blob(idx), blob(dist)
    out[key + ".source"] = blob(ctx.get_source())
    _trace(out, key, ctx.get_trace())
    if robust:
        rt = ctx.get_robust_trace()
        out[key + ".robust_kept"] = blob(np.array([x["kept"] for x in rt], np.int32))
        out[key + ".robust_cut"] = blob(np.array([x["cut"] for x in rt], np.float32))
        out[key + ".robust_c"] = blob(np.array([x["c"] for x in rt], np.float64))
        out[key + ".robust_wsum"] = blob(np.array([x["wsum"] for x in rt], np.float64))


def _reduced(out, key, res):
    out[key + ".sums"] = blob(res[0])
    out[key + ".rest"] = blob(np.array([float(x) for x in res[1:]], np.float64))


def make_nn_probe(mode):
    def probe(ctx, s):
        """a first, unseeded sweep, the plain reduction over it, the source moved, a seeded sweep"""
        settings(ctx)
        clouds(ctx, s)
        out = {}
        i0, d0 = ctx.nn(mode)
        out["first.idx"], out["first.dist"] = blob(i0), blob(d0)
        _reduced(out, "first.reduce", ctx.reduce(max_dist(s)))
        ctx.transform_source(MOVE_R, MOVE_T * np.float32(s["scale"]))
        i1, d1 = ctx.nn(mode)
        out["seeded.idx"], out["seeded.dist"] = blob(i1), blob(d1)
        ia, da = ctx.get_associations()
        out["assoc.idx"], out["assoc.dist"] = blob(ia), blob(da)
        out["source"], out["target"] = blob(ctx.get_source()), blob(ctx.get_target())
        out["sizes"] = blob(np.array([ctx.source_size, ctx.target_size], np.int32))
        return out
    return probe


def other_target(s):
    """the scene's target in reverse order and a little aside: another cloud of the same size over the same source"""
    shift = np.float32([0.02, -0.01, 0.015]) * np.float32(s["scale"])
    return np.ascontiguousarray(s["target"][:, ::-1] + shift[:, None]).astype(np.float32)


RETARGET_MODES = (("filtered", B.NN_FILTERED), ("pruned", B.NN_PRUNED), ("grid", B.NN_GRID))


def probe_retarget(ctx, s):
    """the target replaced between seeded sweeps while the source stays: no set_source, reset_source or align comes
    between, so only the target's own invalidation stands between the old target's matches, indexes and decimated copy
    and the sweep over the new one"""
    settings(ctx)
    out = {}
    for name, mode in RETARGET_MODES:
        clouds(ctx, s)
        ctx.nn(mode, fetch=False)
        ctx.transform_source(MOVE_R, MOVE_T * np.float32(s["scale"]))
        ctx.nn(mode, fetch=False)  # (seeded by the first sweep)
        ctx.set_target(other_target(s))
        i, d = ctx.nn(mode)
        out[name + ".other.idx"], out[name + ".other.dist"] = blob(i), blob(d)
        ctx.set_target(s["target"])
        i, d = ctx.nn(mode)
        out[name + ".back.idx"], out[name + ".back.dist"] = blob(i), blob(d)
    out["source"] = blob(ctx.get_source())
    return out


FLAVOURS = ("reference", "kabsch", "point_to_plane", "plane_to_plane", "colored", "robust")
FIXED_ITERATIONS = 8
THRESHOLD_AT = 3  # the threshold run ends where the fixed run's 4th test stood


def install_flavour(ctx, s, flavour):
    """clouds and whatever the flavour needs, through public calls; returns the alignment's keywords"""
    settings(ctx)
    clouds(ctx, s)
    kw = dict(nn_mode=B.NN_GRID, host_loop=0, max_nn_dist=max_dist(s))
    if flavour == "reference":
        kw["solve"] = B.SOLVE_REFERENCE
    elif flavour == "kabsch":
        kw["solve"] = B.SOLVE_KABSCH
    elif flavour == "robust":
        kw["solve"] = B.SOLVE_KABSCH
        ctx.set_robust(B.ROBUST_HUBER, 1.0, B.SCALE_MEDIAN, 0.9)
    else:
        ctx.estimate_target_normals(radius(s), 5, viewpoint=s["viewpoint"])
        kw["solve"] = P2L
        if flavour == "plane_to_plane":
            ctx.estimate_source_normals(radius(s), 5, viewpoint=s["viewpoint"])
            ctx.set_plane_to_plane(1e-3)
            kw["solve"] = GICP
        if flavour == "colored":
            ctx.set_target_colors(s["target_intensity"])
            ctx.set_source_colors(s["source_intensity"])
            ctx.estimate_target_color_gradients(radius(s), 4)
            ctx.set_colored(True, 0.968)
    return kw


def flavour_hook(ctx, s, flavour):
    """the flavour's single reduction over the last sweep's associations"""
    md = max_dist(s)
    if flavour == "point_to_plane":
        return ctx.reduce_p2l(md)
    if flavour == "plane_to_plane":
        return ctx.reduce_plane_to_plane(md)
    if flavour == "colored":
        return ctx.reduce_colored(md)
    if flavour == "robust":
        return ctx.reduce_weighted(md, B.SOLVE_KABSCH)
    return ctx.reduce(md)


def align_runs(ctx, s, flavour, kw):
    """the two runs of an align probe on an installed context: fixed iterations, then a threshold exit at the mse the
    fixed run saw at its 4th test.  Returns dict(fixed=(T, st, rc), threshold=...) through `collect`."""
    out = {}
    robust = flavour == "robust"
    ctx.nn(B.NN_GRID, fetch=False)
    _reduced(out, "hook", flavour_hook(ctx, s, flavour))
    if flavour in ("point_to_plane", "plane_to_plane", "colored"):
        out["target_normals"] = blob(ctx.get_target_normals())
    if flavour == "plane_to_plane":
        out["source_normals"] = blob(ctx.get_source_normals())
    if flavour == "colored":
        out["gradients"] = blob(ctx.get_target_color_gradients())
    ctx.reset_source()
    _aligned(ctx, out, "fixed", ctx.align(max_iterations=FIXED_ITERATIONS, fixed_iterations=1, **kw), robust)
    tr = ctx.get_trace()
    thr = float(tr[min(THRESHOLD_AT, len(tr) - 1)]["mse"]) if tr else 1e-4
    out["threshold"] = blob(np.float32(thr))
    ctx.reset_source()
    _aligned(ctx, out, "exit", ctx.align(max_iterations=2 * FIXED_ITERATIONS, threshold=thr, **kw), robust)
    return out


def make_align_probe(flavour):
    def probe(ctx, s):
        kw = install_flavour(ctx, s, flavour)
        return align_runs(ctx, s, flavour, kw)
    return probe


def probe_normals(ctx, s):
    settings(ctx)
    clouds(ctx, s)
    out = {}
    ctx.estimate_target_normals(radius(s), 5, viewpoint=s["viewpoint"], keep_moments=True)
    out["target_normals"] = blob(ctx.get_target_normals())
    st = ctx.get_normal_stats()
    out["n"] = blob(np.array([st["n"], st["n_valid"]], np.int32))
    for k in ("count", "curvature", "moments"):
        out[k] = blob(st[k])
    ctx.estimate_source_normals(radius(s), 5, viewpoint=s["viewpoint"])
    out["source_normals"] = blob(ctx.get_source_normals())
    ctx.set_source_normals(s["source_normals"])
    out["source_normals_set"] = blob(ctx.get_source_normals())
    return out


def _groups(out, key, g):
    out[key + ".n"] = blob(np.array([g["n_in"], g["n_out"]], np.int32))
    for k in ("first_index", "count", "out_of_point"):
        out[key + "." + k] = blob(g[k])


def probe_voxel(ctx, s):
    settings(ctx)
    clouds(ctx, s)
    ctx.set_target_normals(s["target_normals"])
    out = {}
    out["target.counts"] = blob(np.array(ctx.voxel_downsample(1, leaf(s), B.VOXEL_CENTROID), np.int32))
    out["target"], out["target_normals"] = blob(ctx.get_target()), blob(ctx.get_target_normals())
    _groups(out, "target.groups", ctx.get_voxel_groups())
    out["source.counts"] = blob(np.array(ctx.voxel_downsample(0, leaf(s), B.VOXEL_FIRST), np.int32))
    out["source"] = blob(ctx.get_source())
    _groups(out, "source.groups", ctx.get_voxel_groups())
    return out


FILTERS = (("statistical", dict(kind=B.FILTER_STATISTICAL, k=8, std_ratio=1.0)),
           ("radius", dict(kind=B.FILTER_RADIUS, min_neighbors=6)))


def filter_kw(s, kw):
    return dict(kw, radius=0.2 * s["scale"]) if kw["kind"] == B.FILTER_RADIUS else kw


def _outliers(out, key, st):
    out[key + ".n"] = blob(np.array([st["n_in"], st["n_out"]], np.int32))
    out[key + ".value"], out[key + ".out_index"], out[key + ".summary"] = blob(st["value"]), blob(st["out_index"]), blob(st["summary"])
    if st["kth"] is not None:
        out[key + ".kth"] = blob(st["kth"])


def probe_filter(ctx, s):
    settings(ctx)
    out = {}
    for name, kw in FILTERS:
        kw = filter_kw(s, kw)
        for which in (0, 1):
            clouds(ctx, s)
            ctx.set_target_normals(s["target_normals"])
            key = f"{name}.{which}"
            out[key + ".stats_only.counts"] = blob(np.array(ctx.remove_outliers(which, stats_only=True, **kw), np.int32))
            _outliers(out, key + ".stats_only", ctx.outlier_stats())
            out[key + ".counts"] = blob(np.array(ctx.remove_outliers(which, **kw), np.int32))
            _outliers(out, key, ctx.outlier_stats())
            out[key + ".cloud"] = blob(ctx.get_target() if which else ctx.get_source())
            if which:
                out[key + ".normals"] = blob(ctx.get_target_normals())
    return out


def probe_color(ctx, s):
    settings(ctx)
    clouds(ctx, s)
    ctx.set_target_normals(s["target_normals"])
    ctx.set_target_colors(s["target_intensity"])
    ctx.set_source_colors(s["source_intensity"])
    ctx.estimate_target_color_gradients(radius(s), 4, keep_sums=True)
    return dict(gradients=blob(ctx.get_target_color_gradients()), sums=blob(ctx.color_gradient_sums()),
                target_colors=blob(ctx.get_target_colors()), source_colors=blob(ctx.get_source_colors()),
                target_normals=blob(ctx.get_target_normals()))


def score_poses_of(s, n=B.SCORE_MAX_POSES):
    """n small motions about the scene's centre, seeded"""
    rng = np.random.default_rng(s["seed"] + 7)
    c = s["target"].astype(np.float64).mean(1)
    T = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        R = synth.rot_xyz_deg(*rng.uniform(-3, 3, 3))
        T[k, :3, :3] = R
        T[k, :3, 3] = c - R @ c + rng.normal(0, 0.03 * s["scale"], 3)
    T[0] = np.eye(4)
    return T.astype(np.float32)


def probe_score(ctx, s):
    settings(ctx)
    clouds(ctx, s)
    T = score_poses_of(s)
    r = ctx.score_poses(T, max_dist(s), keep_assoc=True)
    out = {k: blob(r[k]) for k in ("sums", "inliers", "fitness", "inlier_rmse", "mean_dist", "information")}
    for name, pose in (("first", 0), ("last", T.shape[0] - 1)):
        idx, dist = ctx.score_associations(pose)
        out[name + ".idx"], out[name + ".dist"] = blob(idx), blob(dist)
    r1 = ctx.score_poses(None, max_dist(s))  # the working source as it stands
    out["current.sums"], out["current.inliers"] = blob(r1["sums"]), blob(r1["inliers"])
    return out


GLOBAL = dict(n_hypotheses=6000, seed=3, edge_similarity=0.0)  # every drawn sample is valid: more than one chunk


def probe_fpfh(ctx, s):
    settings(ctx)
    clouds(ctx, s)
    ctx.estimate_target_normals(radius(s), 5, viewpoint=s["viewpoint"])
    ctx.estimate_source_normals(radius(s), 5, viewpoint=s["viewpoint"])
    out = dict(target_normals=blob(ctx.get_target_normals()), source_normals=blob(ctx.get_source_normals()))
    for which, name in ((0, "source"), (1, "target")):
        ctx.compute_fpfh(which, fpfh_radius(s), keep_spfh=True)
        desc, valid = ctx.get_fpfh(which)
        counts, m = ctx.get_spfh(which)
        out[name + ".desc"], out[name + ".valid"] = blob(desc), blob(valid)
        out[name + ".spfh"], out[name + ".m"] = blob(counts), blob(m)
    si, ti, D = ctx.match_features(mutual=True)
    out["match.src"], out["match.tgt"], out["match.D"] = blob(si), blob(ti), blob(D)
    # the run the model follows, then one whose valid hypotheses cross a chunk of SCORE_MAX_POSES
    for key, kw in (("small_global", MODEL_GLOBAL), ("global", GLOBAL)):
        r, rc = ctx.register_global(max_dist=max_dist(s), **kw)
        out[key + ".T"], out[key + ".sums"] = blob(r["T"]), blob(r["sums"])
        out[key + ".rest"] = blob(np.array([rc, r["hypothesis"], r["inliers"], r["n_valid"], r["n_matches"]], np.int64))
    return out


def tsdf_create(ctx, color=True):
    v = TSDF_VOLUME
    return ctx.tsdf_create(dims=v["dims"], voxel=v["voxel"], origin=v["origin"], trunc=v["trunc"],
                           flags=B.TSDF_COLOR if color else 0)


def tsdf_fuse(ctx, s, color=True):
    n = []
    for d, P, img in ((s["depth_tgt"], s["pose_tgt"], s["image_tgt"]), (s["depth_src"], s["pose_src"], s["image_src"])):
        n.append(ctx.tsdf_integrate(d, P, img if color else None, fx=s["fx"], cx=s["cx"]))
    return n


TSDF_ALIGN = dict(solve=P2L, max_iterations=6, max_nn_dist=0.2, nn_mode=B.NN_GRID, fixed_iterations=1)


def probe_tsdf(ctx, s):
    settings(ctx)
    out = {}
    tsdf_create(ctx)
    out["n_updated"] = blob(np.array(tsdf_fuse(ctx, s), np.int32))
    f, w, c = ctx.tsdf_get(intensity=True)
    out["tsdf"], out["weight"], out["intensity"] = blob(f), blob(w), blob(c)
    out["surface.counts"] = blob(np.array(ctx.tsdf_extract_surface(1), np.int32))
    for k, v in ctx.tsdf_get_surface().items():
        out["surface." + k] = blob(v)
    out["mesh.counts"] = blob(np.array(ctx.tsdf_extract_mesh(1), np.int32))
    for k, v in ctx.tsdf_get_mesh().items():
        out["mesh." + k] = blob(v)
    out["raycast.counts"] = blob(np.array(ctx.tsdf_raycast(s["pose_src"], shape=(s["rows"], s["cols"]), fx=s["fx"],
                                                           cx=s["cx"], **RAY_VIEW), np.int32))
    for k, v in ctx.tsdf_get_raycast().items():
        out["raycast." + k] = blob(v)
    ctx.tsdf_raycast_to_target()
    out["ray_target"], out["ray_target_normals"] = blob(ctx.get_target()), blob(ctx.get_target_normals())
    out["ray_target_colors"] = blob(ctx.get_target_colors())
    ctx.set_source(s["source_world"])
    _aligned(ctx, out, "ray_align", ctx.align(**TSDF_ALIGN))
    ctx.tsdf_surface_to_target()
    out["surface_target"], out["surface_target_normals"] = blob(ctx.get_target()), blob(ctx.get_target_normals())
    out["surface_target_colors"] = blob(ctx.get_target_colors())
    # the planes written back as they were read: the lists are dropped, the next extraction finds the same surface
    ctx.tsdf_set(f, w, c)
    out["surface_again.counts"] = blob(np.array(ctx.tsdf_extract_surface(1), np.int32))
    out["surface_again.points"] = blob(ctx.tsdf_get_surface()["points"])
    return out


MAP_ALIGN = dict(max_iterations=5, fixed_iterations=1, solve=B.SOLVE_KABSCH)


def probe_map(ctx, s):
    settings(ctx)
    out = {}
    ctx.map_reset()
    ctx.map_update_points(B.MAP_ADD_CLOUD, s["target"], 180)
    ctx.set_source(s["source"])
    ctx.map_update(B.MAP_ADD_ASSOCIATED, B.MAP_DELTA_CONFIDENCE, B.MAP_FROM_SOURCE)

    def state(key):
        out[key + ".sizes"] = blob(np.array([ctx.map_size(B.MAP_KEYPOINTS), ctx.map_size(B.MAP_POINTS)], np.int32))
        out[key + ".keypoints"], out[key + ".points"] = blob(ctx.map_get_list(B.MAP_KEYPOINTS)), blob(ctx.map_get_list(B.MAP_POINTS))
        out[key + ".certainty"] = blob(ctx.map_get_certainty())  # (the whole grid: 27 MB, compared as bytes)

    state("filled")
    for k, v in zip(("certainty", "occupied", "list", "index"), ctx.map_query(s["source"])):
        out["query." + k] = blob(v)
    for k, v in zip(("dist", "list", "index"), ctx.map_nearest(s["source"])):
        out["nearest." + k] = blob(v)
    ctx.map_lookup_to_target()
    out["lookup_target"] = blob(ctx.get_target())
    _aligned(ctx, out, "dense", ctx.align_to_map_dense(max_nn_dist=0.3, **MAP_ALIGN))
    ctx.set_source(s["source"])
    ctx.map_list_to_target(B.MAP_KEYPOINTS)
    out["list_target"] = blob(ctx.get_target())
    _aligned(ctx, out, "keypoints", ctx.align_to_map(max_nn_dist=0.3, **MAP_ALIGN))
    ctx.set_target(s["target"])
    ctx.map_set_points(B.MAP_FROM_TARGET)
    state("final")  # (after both trackers' updates and the replaced point list)
    return out


def probe_frontend(ctx, s):
    settings(ctx)
    out = {}
    fx, cx, off = s["fx"], s["cx"], s["offset"]
    ds, dt = s["depth_src"], s["depth_tgt"]
    out["filtered_image"] = blob(ctx.filter_depth_image(ds))
    # the pixel-seed path: both frames in one call, the loop straight after
    out["pair.counts"] = blob(np.array(ctx.backproject_pair(ds, dt, R=s["R"], t=s["t"], fx=fx, cx=cx, filter=True), np.int32))
    out["pair.target"] = blob(ctx.get_target())
    _aligned(ctx, out, "pair_align", ctx.align(max_iterations=6, fixed_iterations=1, max_nn_dist=0.3, solve=B.SOLVE_KABSCH))
    # the next frame against the resident one, read from a registered (pinned) buffer
    ring = np.ascontiguousarray(np.stack([dt, ds]))
    ctx.register_host_buffer(ring)
    try:
        out["resident.counts"] = blob(np.array(ctx.backproject_pair(ring[0], None, R=s["R"], t=s["t"], fx=fx, cx=cx, filter=True), np.int32))
        _aligned(ctx, out, "resident_align", ctx.align(max_iterations=4, threshold=1e-7, max_nn_dist=0.3))
    finally:
        ctx.unregister_host_buffer(ring)
    # the separate calls
    out["bp.counts"] = blob(np.array([ctx.backproject(dt, which=1, fx=fx, cx=cx, offset=off),
                                      ctx.backproject_filtered(ds, which=0, fx=fx, cx=cx, offset=off)], np.int32))
    out["bp.target"], out["bp.source"] = blob(ctx.get_target()), blob(ctx.get_source())
    i, d = ctx.nn(B.NN_GRID)
    out["bp.idx"], out["bp.dist"] = blob(i), blob(d)
    out["bpn.count"] = blob(np.int32(ctx.backproject_with_normals(dt, B.NORMALS_CROSS, fx=fx, cx=cx, offset=off)))
    out["bpn.target"], out["bpn.normals"] = blob(ctx.get_target()), blob(ctx.get_target_normals())
    _aligned(ctx, out, "bpn_align", ctx.align(max_iterations=4, fixed_iterations=1, max_nn_dist=0.3, solve=P2L))
    # FAST and the key-point clouds
    gray = ctx.bgr_to_gray(s["bgr"])
    out["gray"] = blob(gray)
    kp, resp = ctx.detect_fast(gray, threshold=FAST_THRESHOLD)
    out["fast.kp"], out["fast.response"] = blob(kp), blob(resp)
    kp3, resp3 = ctx.detect_fast(s["bgr"], threshold=FAST_THRESHOLD, nonmax=False, type=B.FAST_TYPE_9_16)
    out["fast916.kp"], out["fast916.response"] = blob(kp3), blob(resp3)
    ctx.detect_fast(gray, threshold=FAST_THRESHOLD)
    nt = ctx.detected_to_cloud(_full_depth(s, "tgt"), which=1, fx=fx, cx=cx)
    ns = ctx.detected_to_cloud(_full_depth(s, "src"), R=MOVE_R, t=MOVE_T, which=0, fx=fx, cx=cx)
    out["kp.counts"] = blob(np.array([ns, nt], np.int32))
    out["kp.target"], out["kp.source"] = blob(ctx.get_target()), blob(ctx.get_source())
    rc, aq, at, ad, rj = ctx.associate_keypoints(0.1)
    out["kp.rc"] = blob(np.int32(rc))
    if aq is not None:
        out["kp.assoc_q"], out["kp.assoc_t"], out["kp.assoc_d"], out["kp.rejected"] = blob(aq), blob(at), blob(ad), blob(rj)
    return out


@functools.lru_cache(maxsize=None)
def _full_depth_cached(name, which):
    a = SCENE_ARGS[name]
    s = scene(name)
    P = s["pose_tgt"] if which == "tgt" else s["pose_src"]
    d = synth.render_room_depth(a["rows"], a["cols"], P[:3, :3], P[:3, 3], a["fx"], a["cx"])
    d.flags.writeable = False
    return d


def _full_depth(s, which):
    """the scene's frame without the validity mask (a key point needs a depth under it)"""
    return _full_depth_cached(s["name"], which)


def batch_pairs(s):
    """three ragged pairs cut from the scene"""
    src, tgt = s["source"], s["target"]
    ns, nt = src.shape[1], tgt.shape[1]
    cuts = ((ns, nt), (max(ns // 3, 1), max(2 * nt // 3, 1)), (max(ns // 2 + 1, 1), max(nt // 5, 1)))
    return [(src[:, :a].copy(), tgt[:, :b].copy()) for a, b in cuts]


BATCH_ALIGN = dict(max_iterations=5, fixed_iterations=1, solve=B.SOLVE_KABSCH, max_nn_dist=0.3)


def probe_batch(ctx, s):
    import torch

    settings(ctx)
    ctx.release_frame_streams()
    out = {}
    pairs = batch_pairs(s)
    T, st, rc, assoc = ctx.align_batch(pairs, associations=True, **BATCH_ALIGN)
    out["batch.T"], out["batch.rc"] = blob(T), blob(np.int32(rc))
    for b, x in enumerate(st):
        _stats(out, f"batch.{b}", x)
        out[f"batch.{b}.idx"], out[f"batch.{b}.dist"] = blob(assoc[b][0]), blob(assoc[b][1])
    # the same pairs from device memory, and a single cloud pair set from device memory
    keep = [(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()) for a, b in pairs]
    torch.cuda.synchronize()
    Td, std, rcd = ctx.align_batch_device([(a.data_ptr(), a.shape[1], b.data_ptr(), b.shape[1]) for a, b in keep],
                                          B.default_params(**BATCH_ALIGN))
    out["device.T"], out["device.rc"] = blob(Td), blob(np.int32(rcd))
    for b, x in enumerate(std):
        _stats(out, f"device.{b}", x)
    a, b = keep[0]
    ctx.set_target_device(b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b.shape[1])
    ctx.set_source_device(a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a.shape[1])
    _aligned(ctx, out, "device_single", ctx.align(**BATCH_ALIGN))
    ctx.commit_source()
    out["committed"] = blob(ctx.get_source())
    # two streams of the scene's frames over two calls: the second call uses the resident frames
    fx, cx = s["fx"], s["cx"]
    ds, dt = s["depth_src"], s["depth_tgt"]
    frames = dict(fx=fx, cx=cx, max_iterations=5, threshold=1e-7, max_nn_dist=0.3)
    jobs = [dict(stream=0, source=ds, target=dt, R=s["R"], t=s["t"]), dict(stream=5, source=dt, target=ds)]
    for call in ("first", "second"):
        T, st, rc = ctx.align_frames_batch(jobs, **frames)
        out[f"frames.{call}.T"], out[f"frames.{call}.rc"] = blob(T), blob(np.int32(rc))
        for j, x in enumerate(st):
            _stats(out, f"frames.{call}.{j}", x)
            _trace(out, f"frames.{call}.{j}", ctx.get_frames_trace(j))
        jobs = [dict(stream=0, source=dt, target=None, R=s["R"], t=s["t"]), dict(stream=5, source=ds, target=None)]
    return out


PG_CASE = "A"  # the smallest of posegraph_cases' graphs: 8 nodes, one closure; its model is order-insensitive (s_graph 0)


def probe_posegraph(ctx, s):
    import posegraph_cases as pc

    settings(ctx)
    c = pc.case(PG_CASE)
    out = {}
    P, res, w, chi2, pruned, rc = ctx.pose_graph_optimize(c["poses"], c["edges"], **pc.binding_params(c["params"]))
    out["poses"], out["weights"], out["chi2"], out["pruned"] = blob(P), blob(w), blob(chi2), blob(pruned)
    out["result.int"] = blob(np.array([rc, res.iterations, res.accepted, res.pcg_iterations, res.n_pruned], np.int32))
    out["result.float"] = blob(np.array([res.initial_cost, res.final_cost, res.final_lambda], np.float64))
    tr = ctx.get_pose_graph_trace()
    out["trace.cost"], out["trace.lam"] = blob(np.array([x["cost"] for x in tr])), blob(np.array([x["lam"] for x in tr]))
    out["trace.pcg"] = blob(np.array([x["pcg_iterations"] for x in tr], np.int32))
    out["trace.accepted"] = blob(np.array([x["accepted"] for x in tr], np.uint8))
    e_chi2, e_w, cost, g = ctx.pose_graph_evaluate(c["poses"], c["edges"], 0.0)
    out["evaluate.chi2"], out["evaluate.weights"], out["evaluate.gradient"] = blob(e_chi2), blob(e_w), blob(g)
    out["evaluate.cost"] = blob(np.float64(cost))
    return out


PROBES = {}
for _name, _mode in (("nn_exact", B.NN_EXACT), ("nn_filtered", B.NN_FILTERED), ("nn_pruned", B.NN_PRUNED), ("nn_grid", B.NN_GRID)):
    PROBES[_name] = make_nn_probe(_mode)
for _f in FLAVOURS:
    PROBES["align_" + _f] = make_align_probe(_f)
PROBES["retarget"] = probe_retarget
PROBES.update(normals=probe_normals, voxel=probe_voxel, filter=probe_filter, color=probe_color, score=probe_score,
              fpfh=probe_fpfh, tsdf=probe_tsdf, map=probe_map, frontend=probe_frontend, batch=probe_batch,
              posegraph=probe_posegraph)
PROBE_ORDER = tuple(PROBES)
# probes 1-8 of the issue's list: the ones test_shrink_grow_chain runs
CHAIN_PROBES = tuple(k for k in PROBE_ORDER if k not in ("tsdf", "map", "frontend", "batch", "posegraph"))


def run_probes(ctx, s, names=PROBE_ORDER):
    return {k: PROBES[k](ctx, s) for k in names}


# --------------------------------------------------------------------------------------------------- histories --
REFUSALS = (B.E_ARG, B.E_NOT_SET, B.E_EMPTY_TARGET)


def _quiet(fn, *a, **kw):
    """a call whose refusal is part of the history: the statuses the header defines for arguments and missing state
    come back as a value; a device or communicator error (E_HIP, E_RCCL, E_NO_DEVICE) is no history and is raised"""
    try:
        return fn(*a, **kw)
    except B.IcpkError as e:
        if e.code not in REFUSALS:
            raise
        return e.code


def make_scene_history(scene_name, probe_name):
    def history(ctx):
        # (not through _quiet: every probe runs to its end on Q and on S -- the tiny scene's empty key-point clouds and
        # too few matches are statuses the probes record, not refusals -- so a refusal here would cut the history short
        # unseen, and is raised instead)
        PROBES[probe_name](ctx, scene(scene_name))
    return history


class Facts(list):
    """what an early-path history saw of the path it is named for: (label, got, wanted).  The history itself asserts
    nothing; test_gpu_history.py::test_early_history_takes_its_path holds the entries against each other."""

    def note(self, label, got, want):
        self.append((label, got, want))
        return got


def early_far_source(ctx):
    """a source 100 m away: fewer than min_pairs pairs, the fall-back to the caller's last motion (W_TOO_FEW_PAIRS)"""
    s, facts = scene("P"), Facts()
    settings(ctx)
    ctx.set_target(s["target"])
    ctx.set_source(s["source"] + np.float32(100))
    for solve in (B.SOLVE_REFERENCE, B.SOLVE_KABSCH):
        ctx.reset_source()
        T, st, rc = ctx.align(solve=solve, max_iterations=6, fixed_iterations=1, last_translation=np.float32([0.01, 0.02, 0.03]))
        facts.note(f"align solve {solve}", rc, B.W_TOO_FEW_PAIRS)
    return facts


def early_first_threshold_exit(ctx):
    """the loop leaves at its first threshold test while the iterations enqueued ahead of it are still in flight"""
    s, facts = scene("Q"), Facts()
    settings(ctx)
    clouds(ctx, s)
    for solve in (B.SOLVE_KABSCH, B.SOLVE_REFERENCE):
        ctx.reset_source()
        T, st, rc = ctx.align(max_iterations=30, threshold=1e6, solve=solve)
        facts.note(f"iterations solve {solve}", (rc, st.iterations), (B.OK, 0))
    return facts


def early_empty_source(ctx):
    """an empty source through the loop and the calls that read the source"""
    s, facts = scene("P"), Facts()
    settings(ctx)
    ctx.set_target(s["target"])
    ctx.set_source(np.zeros((3, 0), np.float32))
    r = _quiet(ctx.align, max_iterations=4)
    facts.note("align ran", isinstance(r, tuple), True)
    _quiet(ctx.nn, B.NN_GRID)
    r = _quiet(ctx.score_poses, None, 0.1)  # (include/icpk.h: an empty source gives zero sums and zero inliers)
    facts.note("score: no inliers", isinstance(r, dict) and int(r["inliers"][0]), 0)
    _quiet(ctx.voxel_downsample, 0, 0.1)
    facts.note("remove_outliers", _quiet(ctx.remove_outliers, 0), (0, 0))  # (an empty cloud gives an empty cloud)
    return facts


def early_filter_leaves_nothing(ctx):
    """remove_outliers with settings no point meets: both clouds end empty, then the calls that read them"""
    s, facts = scene("P"), Facts()
    settings(ctx)
    clouds(ctx, s)
    ctx.estimate_target_normals(radius(s), 5)
    none = dict(kind=B.FILTER_RADIUS, radius=1e-4, min_neighbors=50)
    facts.note("target left", ctx.remove_outliers(1, **none)[0], 0)
    facts.note("source left", ctx.remove_outliers(0, **none)[0], 0)
    facts.note("align", _quiet(ctx.align, max_iterations=4), B.E_EMPTY_TARGET)
    _quiet(ctx.get_target_normals)
    _quiet(ctx.voxel_downsample, 1, 0.1)
    return facts


def early_small_capacities(ctx):
    """detect_fast and associate_keypoints with a capacity smaller than the result"""
    s, facts = scene("P"), Facts()
    settings(ctx)
    kp, resp = ctx.detect_fast(s["bgr"], threshold=FAST_THRESHOLD, capacity=2)
    facts.note("detect_fast wrote 2 of more", (kp.shape[0], ctx.detected_count > 2), (2, True))
    ctx.detected_to_cloud(_full_depth(s, "tgt"), which=1, fx=s["fx"], cx=s["cx"])
    ctx.detected_to_cloud(_full_depth(s, "src"), which=0, fx=s["fx"], cx=s["cx"])
    _quiet(ctx.associate_keypoints, 1e-6, B.NN_GRID, None, 1)  # (every key point is rejected: more than one entry)
    clouds(ctx, s)
    facts.note("associate_keypoints", _quiet(ctx.associate_keypoints, 1e-6, B.NN_EXACT, None, 3), B.E_ARG)
    return facts


def early_too_few_matches(ctx):
    """register_global with fewer than three matches (W_TOO_FEW_PAIRS, the identity)"""
    s, facts = scene("P"), Facts()
    settings(ctx)
    ctx.set_target(s["target"])
    ctx.set_source(s["source"][:, :2])
    ctx.estimate_target_normals(radius(s), 5)
    ctx.set_source_normals(s["source_normals"][:, :2])
    ctx.compute_fpfh(0, fpfh_radius(s) * 4)
    ctx.compute_fpfh(1, fpfh_radius(s))
    ctx.match_features(mutual=False)
    r, rc = ctx.register_global(n_hypotheses=64, max_dist=0.1)
    facts.note("register_global", (rc, r["hypothesis"]), (B.W_TOO_FEW_PAIRS, -1))
    return facts


def early_refusals(ctx):
    """each feature's E_ARG refusals, issued after its state has been installed"""
    s, facts = scene("P"), Facts()
    settings(ctx)
    clouds(ctx, s)
    ctx.estimate_target_normals(radius(s), 5, keep_moments=True)
    ctx.estimate_source_normals(radius(s), 5)
    ctx.set_target_colors(s["target_intensity"])
    ctx.set_source_colors(s["source_intensity"])
    ctx.estimate_target_color_gradients(radius(s), 4, keep_sums=True)
    ctx.nn(B.NN_GRID, fetch=False)
    ctx.map_reset()
    refused = {
        "nn mode": lambda: ctx.nn(17),
        "align solve": lambda: ctx.align(solve=9),
        "align NN_MAP without a lookup target": lambda: ctx.align(nn_mode=B.NN_MAP),
        "target normals radius": lambda: ctx.estimate_target_normals(-1.0),
        "target normals min_neighbors": lambda: ctx.estimate_target_normals(0.1, 2),
        "source normals radius": lambda: ctx.estimate_source_normals(float("nan")),
        "set_source_normals size": lambda: ctx.set_source_normals(s["source_normals"][:, :5]),
        "set_plane_to_plane": lambda: ctx.set_plane_to_plane(0.0),
        "set_colored lambda": lambda: ctx.set_colored(True, 2.0),
        "set_target_colors range": lambda: ctx.set_target_colors(s["target_intensity"] + np.float32(2)),
        "set_source_colors size": lambda: ctx.set_source_colors(s["source_intensity"][:-1]),
        "gradients min_neighbors": lambda: ctx.estimate_target_color_gradients(0.1, 0),
        "set_robust kernel": lambda: ctx.set_robust(7),
        "set_robust scale": lambda: ctx.set_robust(B.ROBUST_HUBER, -1.0),
        "voxel which": lambda: ctx.voxel_downsample(2, 0.1),
        "voxel leaf": lambda: ctx.voxel_downsample(1, -0.1),
        "filter k": lambda: ctx.remove_outliers(1, k=B.FILTER_MAX_K + 1),
        "filter radius": lambda: ctx.remove_outliers(0, kind=B.FILTER_RADIUS, radius=-1.0),
        "score: more than SCORE_MAX_POSES": lambda: ctx.score_poses(
            np.tile(np.eye(4, dtype=np.float32), (B.SCORE_MAX_POSES + 1, 1, 1)), 0.1),
        "score max_dist": lambda: ctx.score_poses(np.eye(4, dtype=np.float32), -1.0),
        "fpfh which": lambda: ctx.compute_fpfh(2, 0.1),
        "fpfh radius": lambda: ctx.compute_fpfh(1, -0.1),
        "fast type": lambda: ctx.detect_fast(s["bgr"], 20, True, B.FAST_TYPE_5_8),
        "map rule": lambda: ctx.map_update_points(3, s["target"][:, :3], 25),
        "tsdf dims": lambda: ctx.tsdf_create(dims=(0, 4, 4), voxel=0.1, origin=(0, 0, 0), trunc=0.2),
    }
    for label, call in refused.items():
        facts.note(label, _quiet(call), B.E_ARG)
    ctx.compute_fpfh(0, fpfh_radius(s))
    ctx.compute_fpfh(1, fpfh_radius(s))
    ctx.match_features(mutual=True)
    facts.note("global n_hypotheses", _quiet(ctx.register_global, n_hypotheses=0), B.E_ARG)
    facts.note("global edge_similarity", _quiet(ctx.register_global, edge_similarity=1.5), B.E_ARG)
    ctx.set_robust(B.ROBUST_HUBER, 1.0, B.SCALE_MEDIAN, 1.0)
    facts.note("plane-to-plane while robust", _quiet(ctx.align, solve=GICP, max_iterations=2), B.E_ARG)
    ctx.set_colored(True)
    facts.note("colored while robust", _quiet(ctx.align, solve=P2L, max_iterations=2), B.E_ARG)
    ctx.set_robust(None)
    facts.note("colored align_to_map", _quiet(ctx.align_to_map, solve=P2L), B.E_ARG)
    ctx.set_colored(False)
    tsdf_create(ctx)
    facts.note("tsdf_integrate without the intensity",
               _quiet(ctx.tsdf_integrate, s["depth_tgt"], s["pose_tgt"], None, fx=s["fx"], cx=s["cx"]), B.E_ARG)
    facts.note("tsdf min_weight", _quiet(ctx.tsdf_extract_surface, 0), B.E_ARG)
    facts.note("raycast z_near", _quiet(ctx.tsdf_raycast, s["pose_tgt"], shape=(4, 4), fx=4.0, cx=2.0, z_near=-1.0, z_far=3.0), B.E_ARG)
    T, st, rc = ctx.align_frames_batch([dict(stream=B.MAX_FRAME_STREAMS, source=s["depth_src"])], fx=s["fx"], cx=s["cx"])
    facts.note("frames batch stream", rc, B.E_ARG)
    T, st, rc = ctx.align_batch(batch_pairs(s), solve=GICP)
    facts.note("batch plane-to-plane", rc, B.E_ARG)
    return facts


def early_not_set_after_release(ctx):
    """volumes and maps created, reset and released; what they held is gone afterwards"""
    s, facts = scene("P"), Facts()
    settings(ctx)
    tsdf_create(ctx, color=False)
    tsdf_fuse(ctx, s, color=False)
    ctx.tsdf_extract_surface(1)
    ctx.tsdf_reset()
    facts.note("surface of a reset volume", ctx.tsdf_extract_surface(1), (0, 0))
    facts.note("hand-over of an empty list", _quiet(ctx.tsdf_surface_to_target), B.E_EMPTY_TARGET)
    tsdf_fuse(ctx, s, color=False)
    ctx.tsdf_release()
    facts.note("extraction without a volume", _quiet(ctx.tsdf_extract_surface, 1), B.E_NOT_SET)
    ctx.map_reset()
    ctx.map_update_points(B.MAP_ADD_CLOUD, s["target"], 180)
    ctx.map_lookup_to_target()
    ctx.set_source(s["source"])
    ctx.nn(B.NN_MAP, fetch=False)
    ctx.map_release()
    ctx.release_frame_streams()
    return facts


def early_transform_target(ctx):
    """transform_target after normals and gradients exist: both are rotated along, the kept sums are dropped"""
    s, facts = scene("P"), Facts()
    settings(ctx)
    clouds(ctx, s)
    ctx.estimate_target_normals(radius(s), 5, keep_moments=True)
    ctx.set_target_colors(s["target_intensity"])
    ctx.estimate_target_color_gradients(radius(s), 4, keep_sums=True)
    ctx.compute_fpfh(1, fpfh_radius(s))
    ctx.nn(B.NN_GRID, fetch=False)
    ctx.transform_target(MOVE_R, MOVE_T)
    facts.note("kept sums", _quiet(ctx.color_gradient_sums), B.E_NOT_SET)
    facts.note("gradients stay", isinstance(_quiet(ctx.get_target_color_gradients), np.ndarray), True)
    ctx.nn(B.NN_GRID, fetch=False)
    ctx.align(solve=P2L, max_iterations=3)
    return facts


def early_commit_with_records_pending(ctx):
    """commit_source straight after a device-loop alignment (the loop's records not yet unpacked into the working
    source), then a sweep and a second alignment from the committed cloud"""
    s, facts = scene("P"), Facts()
    settings(ctx)
    clouds(ctx, s)
    T, st, rc = ctx.align(max_iterations=5, fixed_iterations=1, solve=B.SOLVE_KABSCH)
    facts.note("device loop ran", (rc, st.iterations), (B.OK, 5))
    ctx.commit_source()
    ctx.nn(B.NN_GRID, fetch=False)
    ctx.align(max_iterations=3, fixed_iterations=1)
    ctx.commit_source()
    ctx.reset_source()
    return facts


def non_finite_cloud(s):
    pts = s["target"].copy()
    pts[0, 5], pts[1, 70], pts[2, 1100] = np.nan, np.inf, -np.inf
    pts[:, 1500] = np.nan
    return pts


def early_non_finite(ctx):
    """a cloud with NaN and infinite points through K12, K13, K16 and K17 only (see the module's docstring)"""
    s, facts = scene("P"), Facts()
    settings(ctx)
    bad = non_finite_cloud(s)
    ctx.set_target(bad)
    ctx.set_source(bad[:, :1600])
    ctx.estimate_target_normals(radius(s), 5, keep_moments=True)
    ctx.estimate_source_normals(radius(s), 5)
    ctx.set_target_colors(s["target_intensity"])
    ctx.estimate_target_color_gradients(radius(s), 4, keep_sums=True)
    ctx.compute_fpfh(0, fpfh_radius(s), keep_spfh=True)
    ctx.compute_fpfh(1, fpfh_radius(s), keep_spfh=True)
    ctx.match_features(mutual=True)
    for name, kw in FILTERS:
        ctx.remove_outliers(1, stats_only=True, **filter_kw(s, kw))
    facts.note("dropped from the target", ctx.remove_outliers(1, **filter_kw(s, FILTERS[0][1]))[1], 4)
    facts.note("dropped from the source", ctx.remove_outliers(0, **filter_kw(s, FILTERS[1][1]))[1], 4)
    return facts


def early_one_rank_communicator(ctx):
    """the RCCL calls on a communicator of one rank (tests/test_gpu_comm.py builds the same)"""
    from icp_slam_prototype_amd import batch

    s, facts = scene("P"), Facts()
    settings(ctx)
    clouds(ctx, s)
    comm = batch.RcclComm(ctx, 0, 1, lambda uid: uid)
    try:
        facts.note("rank and world", (ctx.comm_rank, ctx.comm_world), (0, 1))
        ctx.nn(B.NN_GRID, fetch=False)
        ctx.comm_broadcast_target(0)
        T, st, rc = ctx.align_batch(batch_pairs(s), **BATCH_ALIGN)
        ctx.comm_gather_results(T, st, len(st))
        ctx.comm_allreduce_sums(np.arange(19, dtype=np.float64), 5)
        ctx.comm_barrier()
        ctx.reset_source()
        ctx.align_query_sharded(max_iterations=4, solve=B.SOLVE_KABSCH, fixed_iterations=1)
    finally:
        comm.close()
    facts.note("world afterwards", ctx.comm_world, 0)
    return facts


EARLY = {
    "early_far_source": early_far_source,
    "early_first_threshold_exit": early_first_threshold_exit,
    "early_empty_source": early_empty_source,
    "early_filter_leaves_nothing": early_filter_leaves_nothing,
    "early_small_capacities": early_small_capacities,
    "early_too_few_matches": early_too_few_matches,
    "early_refusals": early_refusals,
    "early_not_set_after_release": early_not_set_after_release,
    "early_transform_target": early_transform_target,
    "early_commit_with_records_pending": early_commit_with_records_pending,
    "early_non_finite": early_non_finite,
    "early_one_rank_communicator": early_one_rank_communicator,
}

def shared_aux_index(ctx):
    """the context's one index of "any other cloud" (csrc/icpk_ctx.h: aux_grid) as its OTHER user left it: on Q the
    source normals index the uploaded source, then the filter's statistics index the working source -- the last call
    that builds an index.  The probes on P then find that index holding a larger cloud with another bounding box."""
    s = scene("Q")
    settings(ctx)
    clouds(ctx, s)
    ctx.estimate_source_normals(radius(s), 5, viewpoint=s["viewpoint"])
    ctx.remove_outliers(0, stats_only=True, **filter_kw(s, FILTERS[0][1]))


# histories that hand a piece of state two features share from one to the other
SHARED = {"shared_aux_index": shared_aux_index}

HISTORIES = {}
for _s in ("Q", "S"):
    for _p in PROBE_ORDER:
        HISTORIES[f"{_s}.{_p}"] = make_scene_history(_s, _p)
HISTORIES.update(EARLY)
HISTORIES.update(SHARED)


# ------------------------------------------------------------------------------------------------------ models --
# What the independent models the suite owns say about a probe on a scene.  Each returns dict(key -> array) of the
# probe's keys the model gives bit for bit (tests/test_gpu_history.py compares bytes), and may add "facts": figures
# the host test reads for its soundness check.  Inputs that reach the device through a chain the feature's own test
# holds only to a tolerance (estimated normals: tests/test_gpu_normals.py::_check, 1e-6 rad) are taken from the fresh
# probe's own output (`given`), so that what follows them can still be compared bit for bit; on the host the model's
# own normals stand in.
def unblob(b):
    return np.frombuffer(b, b.dtype).reshape(b.shape)


def _model_normals(pts, s):
    import normals_model as nm

    return nm.estimate(pts, radius(s), 5, s["viewpoint"])


def model_nn(s, oracle, given=None):
    scale = np.float32(s["scale"])
    i0, d0 = oracle.nn_bruteforce(s["source"], s["target"])
    moved = oracle.transform_points(s["source"], MOVE_R, MOVE_T * scale)
    i1, d1 = oracle.nn_bruteforce(moved, s["target"])
    return {"first.idx": i0, "first.dist": d0, "seeded.idx": i1, "seeded.dist": d1, "assoc.idx": i1, "assoc.dist": d1,
            "source": moved, "target": s["target"], "facts": dict(near=int((d0 < max_dist(s)).sum()))}


def model_retarget(s, oracle, given=None):
    moved = oracle.transform_points(s["source"], MOVE_R, MOVE_T * np.float32(s["scale"]))
    io, do = oracle.nn_bruteforce(moved, other_target(s))
    ib, db = oracle.nn_bruteforce(moved, s["target"])
    out = {"source": moved, "facts": dict(changed=int((io != ib).sum()))}
    for name, _ in RETARGET_MODES:
        out[name + ".other.idx"], out[name + ".other.dist"] = io, do
        out[name + ".back.idx"], out[name + ".back.dist"] = ib, db
    return out


def model_hook(s, oracle, flavour, given=None):
    """the flavour's single reduction over the first sweep (K5, K14, K17 through the canonical tree, bit for bit; the
    robust selection -- cut, median, c, counts -- exactly, its sums only to the tree's rounding and so not here:
    tests/test_gpu_robust.py::check_reduce_weighted)"""
    import color_model as cm
    import gicp_model as gm
    import robust_model as rm

    src, tgt, md = s["source"], s["target"], max_dist(s)
    idx, dist = oracle.nn_bruteforce(src, tgt)
    given = given or {}
    out = {}
    if flavour in ("point_to_plane", "plane_to_plane", "colored"):
        tn = given.get("target_normals")
        tn = _model_normals(tgt, s)["normals"] if tn is None else tn
    if flavour == "point_to_plane":
        sums, cnt = oracle.sums_p2l_canonical(src, tgt, tn, idx, dist, md)  # (tests/test_gpu_parity.py holds K5 to it)
    elif flavour == "plane_to_plane":
        sn = given.get("source_normals")
        sn = _model_normals(src, s)["normals"] if sn is None else sn
        sums, cnt = gm.sums(src, tgt, sn, tn, idx, dist, md, 1e-3)
    elif flavour == "colored":
        g = given.get("gradients")
        g = cm.gradients(tgt, tn, s["target_intensity"], radius(s), 4)[0] if g is None else g
        sums, cnt = cm.sums(src, tgt, tn, g, s["target_intensity"], s["source_intensity"], idx, dist, md, 0.968)
    elif flavour == "robust":
        cfg = dict(kernel=rm.HUBER, scale=1.0, scale_mode=rm.MEDIAN, trim=0.9)
        acc, w, tau, m, c = rm.robust_weights(dist, md, cfg)
        rest = np.array([float(np.count_nonzero(acc)), float(np.count_nonzero(w > 0)), float(np.float32(tau)),
                         float(np.float32(m)), float(c)], np.float64)
        return {"hook.rest": rest, "facts": dict(accepted=int(acc.sum()), kept=int((w > 0).sum()))}
    else:
        return {"facts": dict(accepted=int((dist < np.float32(md)).sum()))}
    out["hook.sums"], out["hook.rest"] = sums, np.array([float(cnt)], np.float64)
    out["facts"] = dict(accepted=cnt)
    return out


def model_normals(s, oracle=None, given=None):
    """count and moments bit for bit; the normals themselves are held to tests/test_gpu_normals.py::_check's 1e-6 rad
    by the GPU test, which calls that function"""
    t, q = _model_normals(s["target"], s), _model_normals(s["source"], s)
    return {"count": t["count"].astype(np.int32), "moments": t["moments"].astype(np.int64),
            "source_normals_set": s["source_normals"],
            "facts": dict(n=s["target"].shape[1], target_valid=int(t["n_valid"]), source_valid=int(q["n_valid"]))}


def model_voxel(s, oracle=None, given=None):
    import voxel_model as vm

    t = vm.downsample(s["target"], leaf(s), vm.CENTROID, s["target_normals"])
    q = vm.downsample(s["source"], leaf(s), vm.FIRST)
    out = {"target": t["points"], "target_normals": t["normals"], "source": q["points"],
           "target.counts": np.array([t["n_out"], t["n_dropped"]], np.int32),
           "source.counts": np.array([q["n_out"], q["n_dropped"]], np.int32)}
    for name, r, n_in in (("target", t, s["target"].shape[1]), ("source", q, s["source"].shape[1])):
        out[name + ".groups.n"] = np.array([n_in, r["n_out"]], np.int32)
        for k in ("first_index", "count", "out_of_point"):
            out[f"{name}.groups.{k}"] = np.asarray(r[k], np.int32)
    out["facts"] = dict(target_out=int(t["n_out"]), source_out=int(q["n_out"]))
    return out


def model_filter(s, oracle=None, given=None):
    import filter_model as fm

    out, facts = {}, {}
    for name, kw in FILTERS:
        kw = filter_kw(s, kw)
        for which in (0, 1):
            pts = s["target"] if which else s["source"]
            m = fm.remove_outliers(pts, normals=s["target_normals"] if which else None, **kw)
            key = f"{name}.{which}"
            for pre in (key + ".stats_only", key):
                out[pre + ".value"], out[pre + ".out_index"], out[pre + ".summary"] = m["value"], m["out_index"], m["summary"]
                out[pre + ".n"] = np.array([pts.shape[1], m["n_out"]], np.int32)
                if m["kth"] is not None:
                    out[pre + ".kth"] = m["kth"]
            out[key + ".counts"] = np.array([m["n_out"], m["n_dropped"]], np.int32)
            out[key + ".cloud"] = m["points"]
            if which:
                out[key + ".normals"] = m["normals"]
            facts[key] = (pts.shape[1], int(m["n_out"]))
    out["facts"] = facts
    return out


def model_color(s, oracle=None, given=None):
    import color_model as cm

    g, S = cm.gradients(s["target"], s["target_normals"], s["target_intensity"], radius(s), 4)
    return {"gradients": g, "sums": S, "target_colors": s["target_intensity"], "source_colors": s["source_intensity"],
            "target_normals": s["target_normals"], "facts": dict(with_gradient=int((g != 0).any(0).sum()))}


SCORE_MODEL_POSES = (0, 1, B.SCORE_MAX_POSES // 2, B.SCORE_MAX_POSES - 1)


def model_score(s, oracle=None, given=None):
    """the poses of SCORE_MODEL_POSES (the model is quadratic in the cloud: four of the 4096 are held against it)"""
    import score_model as sm

    T = score_poses_of(s)
    rows = {k: sm.score(s["source"], s["target"], T[k], max_dist(s)) for k in SCORE_MODEL_POSES}
    out = {"rows": rows, "first.idx": rows[0]["idx"], "first.dist": rows[0]["dist"],
           "last.idx": rows[SCORE_MODEL_POSES[-1]]["idx"], "last.dist": rows[SCORE_MODEL_POSES[-1]]["dist"],
           "current.sums": rows[0]["sums"][None], "current.inliers": np.array([rows[0]["inliers"]], np.int64)}
    out["facts"] = dict(inliers=[int(r["inliers"]) for r in rows.values()])
    return out


MODEL_GLOBAL = dict(n_hypotheses=64, seed=3, edge_similarity=0.6)  # (the model scores every valid hypothesis on the CPU)


def model_fpfh(s, oracle=None, given=None):
    import fpfh_model as fm

    given = given or {}
    tn, sn = given.get("target_normals"), given.get("source_normals")
    tn = _model_normals(s["target"], s)["normals"] if tn is None else tn
    sn = _model_normals(s["source"], s)["normals"] if sn is None else sn
    fs, ft = fm.fpfh(s["source"], sn, fpfh_radius(s)), fm.fpfh(s["target"], tn, fpfh_radius(s))
    si, ti, D = fm.match(fs["desc"], fs["valid"], ft["desc"], ft["valid"], mutual=True)
    g = fm.register_global((si, ti), s["source"], s["target"], MODEL_GLOBAL["n_hypotheses"], MODEL_GLOBAL["seed"],
                           max_dist(s), MODEL_GLOBAL["edge_similarity"])
    out = {"match.src": si, "match.tgt": ti, "match.D": D, "small_global.T": g["T"], "small_global.sums": g["sums"],
           "small_global.rest": np.array([B.OK if g["ok"] else B.W_TOO_FEW_PAIRS, g["hypothesis"], g["inliers"], g["n_valid"],
                                          g["n_matches"]], np.int64)}
    for name, f in (("source", fs), ("target", ft)):
        out[name + ".desc"], out[name + ".valid"] = f["desc"], f["valid"]
        out[name + ".spfh"], out[name + ".m"] = f["counts"], f["m"]
    # the large run: how many of its hypotheses are valid (the draw and the edge test alone; nothing is scored here)
    large = sum(bool(fm.hypothesis((si, ti), s["source"], s["target"], GLOBAL["seed"], GLOBAL["edge_similarity"], h)[1])
                for h in range(GLOBAL["n_hypotheses"])) if len(si) >= 3 else 0
    out["facts"] = dict(matches=len(si), ok=bool(g["ok"]), inliers=int(g["inliers"]), n_valid=int(g["n_valid"]), large_n_valid=large,
                        valid=(int(fs["valid"].sum()), int(ft["valid"].sum())))
    return out


def model_tsdf(s, oracle=None, given=None):
    import tsdf_mesh_model
    import tsdf_model
    import tsdf_raycast_model

    vol = tsdf_model.Volume(color=True, **TSDF_VOLUME)
    n = [vol.integrate(d, P, s["fx"], s["cx"], img) for d, P, img in
         ((s["depth_tgt"], s["pose_tgt"], s["image_tgt"]), (s["depth_src"], s["pose_src"], s["image_src"]))]
    surf = vol.extract(1)
    mesh = tsdf_mesh_model.mesh(vol, 1)
    ray = tsdf_raycast_model.raycast(vol, s["pose_src"], (s["rows"], s["cols"]), s["fx"], s["cx"], **RAY_VIEW)
    out = {"n_updated": np.array(n, np.int32), "tsdf": vol.tsdf, "weight": vol.weight, "intensity": vol.intensity,
           "surface.counts": np.array([surf["points"].shape[1], surf["n_no_normal"]], np.int32),
           "mesh.counts": np.array([mesh["n_vertices"], mesh["n_triangles"], mesh["n_no_normal"]], np.int32),
           "raycast.counts": np.array([ray["n_hits"], ray["n_no_normal"]], np.int32),
           "raycast.points": ray["maps"][0:3], "raycast.normals": ray["maps"][3:6], "raycast.depth": ray["maps"][6],
           "raycast.intensity": ray["maps"][7], "surface_target": surf["points"], "surface_target_normals": surf["normals"],
           "surface_target_colors": surf["intensity"], "surface_again.points": surf["points"]}
    for k in ("points", "normals", "intensity", "voxel", "axis"):
        out["surface." + k] = surf[k]
    for k in ("vertices", "normals", "intensity", "voxel_index", "edge", "triangles"):
        out["mesh." + k] = mesh[k]
    out["facts"] = dict(updated=n, surface=int(surf["points"].shape[1]), triangles=int(mesh["n_triangles"]),
                        hits=int(ray["n_hits"]))
    return out


def model_map(s, oracle=None, given=None):
    """the map after the two updates (state `filled`)"""
    import map_model as mm

    m = mm.Map()
    m.update(mm.ADD_CLOUD, s["target"], 180)
    m.update(mm.ADD_ASSOCIATED, s["source"], B.MAP_DELTA_CONFIDENCE)
    g = m.grid()
    kp, pts = m.list_array(mm.KEYPOINTS), m.list_array(mm.POINTS)
    return {"filled.sizes": np.array([kp.shape[1], pts.shape[1]], np.int32), "filled.keypoints": kp, "filled.points": pts,
            "filled.certainty": g,
            "facts": dict(keypoints=int(kp.shape[1]), points=int(pts.shape[1]), voxels=int(np.count_nonzero(g)))}


def model_frontend(s, oracle=None, given=None):
    import fast_model as fm

    gray = fm.bgr_to_gray(s["bgr"])
    kp, resp = fm.detect(gray, FAST_THRESHOLD, True, fm.TYPE_7_12)
    kp3, resp3 = fm.detect(s["bgr"], FAST_THRESHOLD, False, fm.TYPE_9_16)
    return {"gray": gray, "fast.kp": kp, "fast.response": resp, "fast916.kp": kp3, "fast916.response": resp3,
            "facts": dict(corners=int(len(kp)), corners916=int(len(kp3)))}


def model_posegraph(s=None, oracle=None, given=None):
    """tests/test_gpu_posegraph.py::_compare holds the device within 16 x s_graph of this; nothing bit for bit"""
    import posegraph_cases as pc

    want = pc.model_result(PG_CASE)
    return {"facts": dict(iterations=int(want["iterations"]), final_cost=float(want["final_cost"])), "want": want}


MODELS = {k: model_nn for k in ("nn_exact", "nn_filtered", "nn_pruned", "nn_grid")}


def _hook_model(flavour):
    def model(s, oracle=None, given=None):
        return model_hook(s, oracle, flavour, given)
    return model


for _f in FLAVOURS:
    MODELS["align_" + _f] = _hook_model(_f)
MODELS["retarget"] = model_retarget
MODELS.update(normals=model_normals, voxel=model_voxel, filter=model_filter, color=model_color, score=model_score,
              fpfh=model_fpfh, tsdf=model_tsdf, map=model_map, frontend=model_frontend, posegraph=model_posegraph)
# `batch` has no numpy model: the GPU test holds it against the same pairs one by one (tools' soak_batch does the same)


# ------------------------------------------------------------------------------------------ completeness table --
class Exempt(str):
    """EXEMPT with its reason"""


def EXEMPT(reason):
    return Exempt(reason)


_NO_STATE = "holds no device state of the context"
_ALL_ALIGN = tuple("align_" + f for f in FLAVOURS)
_ALL_NN = ("nn_exact", "nn_filtered", "nn_pruned", "nn_grid")
_COMM = ("early_one_rank_communicator",)

COVERAGE = {
    "close": EXEMPT(_NO_STATE), "stream": EXEMPT(_NO_STATE), "source_size": EXEMPT(_NO_STATE),
    "target_size": EXEMPT(_NO_STATE), "pair_distance": EXEMPT(_NO_STATE), "set_log_callback": EXEMPT(_NO_STATE),
    "set_target": _ALL_NN + ("retarget",), "set_source": _ALL_NN, "set_target_device": ("batch",), "set_source_device": ("batch",),
    "reset_source": _ALL_ALIGN, "commit_source": ("batch", "early_commit_with_records_pending"),
    "get_source": _ALL_NN + _ALL_ALIGN, "get_target": _ALL_NN, "nn": _ALL_NN + ("retarget",), "get_associations": _ALL_NN + _ALL_ALIGN,
    "reduce": _ALL_NN, "transform_source": _ALL_NN, "transform_target": ("early_transform_target",),
    "get_trace": _ALL_ALIGN, "get_frames_trace": ("batch",),
    "register_host_buffer": ("frontend",), "unregister_host_buffer": ("frontend",),
    "set_subsample": PROBE_ORDER, "backproject": ("frontend",), "filter_depth_image": ("frontend",),
    "backproject_filtered": ("frontend",), "backproject_pair": ("frontend",), "align_frames_batch": ("batch",),
    "release_frame_streams": ("batch",), "associate_keypoints": ("frontend", "early_small_capacities"),
    "backproject_with_normals": ("frontend",), "set_target_normals": ("voxel", "filter", "color"),
    "get_target_normals": ("normals", "voxel", "tsdf"), "reduce_p2l": ("align_point_to_plane",),
    "set_robust": PROBE_ORDER, "get_robust_trace": ("align_robust",), "reduce_weighted": ("align_robust",),
    "voxel_downsample": ("voxel",), "get_voxel_groups": ("voxel",),
    "estimate_target_normals": ("normals", "align_point_to_plane", "fpfh"), "get_normal_stats": ("normals",),
    "remove_outliers": ("filter", "early_filter_leaves_nothing", "shared_aux_index"), "outlier_stats": ("filter",),
    "estimate_source_normals": ("normals", "align_plane_to_plane", "fpfh", "shared_aux_index"), "set_source_normals": ("normals",),
    "get_source_normals": ("normals",), "set_plane_to_plane": PROBE_ORDER,
    "reduce_plane_to_plane": ("align_plane_to_plane",),
    "set_target_colors": ("color", "align_colored"), "set_source_colors": ("color", "align_colored"),
    "get_target_colors": ("color", "tsdf"), "get_source_colors": ("color",),
    "estimate_target_color_gradients": ("color", "align_colored"), "get_target_color_gradients": ("color",),
    "color_gradient_sums": ("color",), "set_colored": PROBE_ORDER, "reduce_colored": ("align_colored",),
    "score_poses": ("score",), "score_associations": ("score",),
    "compute_fpfh": ("fpfh",), "get_fpfh": ("fpfh",), "get_spfh": ("fpfh",), "match_features": ("fpfh",),
    "register_global": ("fpfh", "early_too_few_matches"),
    "pose_graph_optimize": ("posegraph",), "pose_graph_evaluate": ("posegraph",), "get_pose_graph_trace": ("posegraph",),
    "tsdf_create": ("tsdf",), "tsdf_reset": ("early_not_set_after_release",), "tsdf_release": ("early_not_set_after_release",),
    "tsdf_integrate": ("tsdf",), "tsdf_get": ("tsdf",), "tsdf_set": ("tsdf",), "tsdf_extract_mesh": ("tsdf",),
    "tsdf_get_mesh": ("tsdf",), "tsdf_extract_surface": ("tsdf",), "tsdf_get_surface": ("tsdf",),
    "tsdf_surface_to_target": ("tsdf",), "tsdf_raycast": ("tsdf",), "tsdf_get_raycast": ("tsdf",),
    "tsdf_raycast_to_target": ("tsdf",), "align": _ALL_ALIGN + ("tsdf", "frontend", "batch"),
    "map_reset": ("map",), "map_release": ("early_not_set_after_release",), "map_update": ("map",),
    "map_update_points": ("map",), "map_set_points": ("map",), "map_size": ("map",), "map_get_list": ("map",),
    "map_get_certainty": ("map",), "map_query": ("map",), "map_list_to_target": ("map",), "align_to_map": ("map",),
    "map_nearest": ("map",), "map_lookup_to_target": ("map",), "align_to_map_dense": ("map",),
    "bgr_to_gray": ("frontend",), "detect_fast": ("frontend", "early_small_capacities"),
    "detected_to_cloud": ("frontend", "early_small_capacities"),
    "align_query_sharded": _COMM, "align_batch": ("batch",), "align_batch_device": ("batch",),
    "comm_init": _COMM, "comm_destroy": _COMM, "comm_rank": _COMM, "comm_world": _COMM, "comm_broadcast_target": _COMM,
    "comm_gather_results": _COMM, "comm_allreduce_sums": _COMM, "comm_barrier": _COMM,
}
