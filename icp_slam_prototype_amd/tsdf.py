"""The model the poses are for (K19): a dense volume of truncated signed distances on the device, into which posed
depth frames are fused (Context.tsdf_integrate) and from which the surface comes back as points with normals
(Context.tsdf_extract_surface) -- or goes on to be the context's target for scan-to-model alignment.

    vol = TsdfVolume(ctx, dims=(256, 256, 256), voxel=0.02, origin=(-2.56, -2.56, 0.0), trunc=0.08)
    vol.integrate_all(depths, graph.poses())   # the optimised poses of posegraph.PoseGraph, camera-to-world
    model = vol.surface(min_weight=2)          # dict(points, normals, intensity, voxel, axis)
    vol.to_target()                            # ... or: the next frame is aligned against the model

The model seen from one pose (K20) -- vertex and normal maps of the visible surface, at the cost of the image and not of
the model -- and the tracking loop it closes:

    view = vol.raycast(pose, shape=(480, 640))  # dict(points (3, rows, cols), normals, depth, intensity, n_hits, ...)
    tracker = ModelTracker(vol, pose=first_pose)
    for depth in frames:
        pose = tracker.track(depth)             # ray-cast at the last pose, align the frame, integrate it

The model as something to keep (K21) -- a triangle mesh, consistently oriented and closed inside the known cells (it is
open where the surface leaves them or the volume), extracted on the device:

    mesh = vol.mesh(min_weight=2)               # dict(vertices (3, n), normals, intensity, ..., triangles (m, 3))
    write_ply("model.ply", mesh)

A scene larger than the box (K23) -- the volume follows the camera by whole voxels, and what is about to fall off is
streamed out first as points with normals:

    tracker = ModelTracker(vol, pose=first_pose, follow=16)   # shift once the camera has moved 16 voxels
    for depth in frames:
        pose = tracker.track(depth)
    parts = tracker.streamed + [vol.surface()]                # the model: what left, and what the box still holds

A tracker that finds the camera again (K27) -- every frame it believes is encoded as a fern code and harvested as a
keyframe when it is new enough; a frame it cannot place is not fused, and the next ones restart from the nearest
keyframes' poses:

    tracker = ModelTracker(vol, pose=first_pose, projective=True, pyramid=(10, 5, 4), relocalise=True)
    for depth in frames:
        pose = tracker.track(depth)
        if tracker.lost: ...                                  # the pose is the last believed one; nothing was fused
"""
import numpy as np

from . import binding, depth as depth_front


class TsdfVolume:
    """The TSDF volume of one Context (a context holds one: creating another replaces it).  fx, cx: the depth camera's
    intrinsics, those Context.backproject takes."""

    def __init__(self, ctx, dims, voxel, origin, trunc, max_weight=None, depth_scale=None, color=False, fx=468.60,
                 cx=318.27, shape=None):
        self.ctx = ctx
        self.shape = shape  # (rows, cols) of the frames: integrate_resident's default, kept up to date by integrate
        self.fx, self.cx = float(fx), float(cx)
        self.params = ctx.tsdf_create(dims=dims, voxel=voxel, origin=origin, trunc=trunc, max_weight=max_weight,
                                      depth_scale=depth_scale, flags=binding.TSDF_COLOR if color else 0)
        self.frames = 0
        self.n_points = self.n_no_normal = None
        self.total = np.zeros(3, np.int64)  # the cumulative shift (K23); params.origin is kept up to date with it
        self.follow_ref = None              # follow()'s reference camera centre: the first pose it sees
        self.follow_min_weight = 1          # ... and the min_weight of the leaving lists it extracts

    def integrate(self, depth, pose, intensity=None):
        """One (rows, cols) uint16 frame at the camera-to-world pose (4, 4).  Returns the number of voxels written."""
        n = self.ctx.tsdf_integrate(depth, pose, intensity, fx=self.fx, cx=self.cx)
        self.shape = tuple(np.shape(depth))
        self.frames += 1
        return n

    def integrate_resident(self, pose, shape=None, intensity=None, count=False):
        """The frame Context.backproject_pair has just left on the device (its filtered copy when the filter was on),
        without a second upload.  shape: its (rows, cols) (default: the last integrated frame's, or the constructor's)."""
        shape = self.shape if shape is None else shape
        if shape is None:
            raise ValueError("the resident frame's (rows, cols) is not known: pass shape")
        n = self.ctx.tsdf_integrate(None, pose, intensity, fx=self.fx, cx=self.cx, shape=shape, count=count)
        self.frames += 1
        return n

    def integrate_all(self, depths, poses, intensities=None):
        """Frames and their poses, e.g. PoseGraph.poses().  Returns the voxels written per frame."""
        poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
        if len(depths) != poses.shape[0] or (intensities is not None and len(intensities) != len(depths)):
            raise ValueError("one pose (and one intensity image) per depth frame")
        return [self.integrate(d, poses[k], None if intensities is None else intensities[k])
                for k, d in enumerate(depths)]

    def deintegrate(self, depth, pose, intensity=None):
        """The inverse of integrate (K30): the frame taken out again at the pose it was fused at.  Exact on voxels the
        frame alone had written, up to rounding elsewhere, and no inverse on voxels that reached max_weight.  Returns
        the number of voxels written."""
        n = binding.tsdf_deintegrate(self.ctx, depth, pose, intensity, fx=self.fx, cx=self.cx)
        self.frames = max(self.frames - 1, 0)  # (a count of calls, not of content: it never goes below 0)
        return n

    def apply(self, frames, ops, intensities=None):
        """Signed updates in one pass over the volume (K30): ops is a list of (sign, frame, pose) -- +1 integrates and -1
        de-integrates frames[frame] at pose --, at most binding.TSDF_MAX_OPS of them over at most as many frames.  Returns
        the voxels every op wrote."""
        n = binding.tsdf_apply(self.ctx, frames, ops, intensities, fx=self.fx, cx=self.cx)
        self.shape = tuple(np.shape(frames[0]))
        self.frames = max(self.frames + sum(int(op[0]) for op in ops), 0)  # (calls, as in deintegrate)
        return n

    REFUSE_BATCH = 8  # frames per call of refuse: two ops each, binding.TSDF_MAX_OPS in all

    def refuse(self, depths, old_poses, new_poses, intensities=None):
        """Frames fused at old_poses moved to new_poses (e.g. PoseGraph.poses() after a loop closure): each is taken out
        at its old pose and put in at its new one, REFUSE_BATCH frames per pass over the volume, every frame uploaded
        once.  Returns the voxels written, (n, 2) int64: removed, added."""
        old = np.asarray(old_poses, np.float64).reshape(-1, 4, 4)
        new = np.asarray(new_poses, np.float64).reshape(-1, 4, 4)
        if not (len(depths) == old.shape[0] == new.shape[0]) or (intensities is not None and len(intensities) != len(depths)):
            raise ValueError("an old pose, a new pose (and an intensity image) per depth frame")
        out = np.zeros((len(depths), 2), np.int64)
        for lo in range(0, len(depths), self.REFUSE_BATCH):
            hi = min(lo + self.REFUSE_BATCH, len(depths))
            ops = [(-1, k - lo, old[k]) for k in range(lo, hi)] + [(+1, k - lo, new[k]) for k in range(lo, hi)]
            n = self.apply(depths[lo:hi], ops, None if intensities is None else intensities[lo:hi])
            out[lo:hi, 0], out[lo:hi, 1] = n[:hi - lo], n[hi - lo:]
        return out

    def surface(self, min_weight=1):
        """The zero crossings between voxels of weight >= min_weight: dict(points (3, n), normals (3, n), intensity,
        voxel, axis), ordered by voxel then axis."""
        self.n_points, self.n_no_normal = self.ctx.tsdf_extract_surface(min_weight)
        return self.ctx.tsdf_get_surface()

    def to_target(self, min_weight=None):
        """The surface list becomes the context's target, with its normals (and colours): device to device.
        min_weight: extract first (else the last extraction's list)."""
        if min_weight is not None or self.n_points is None:
            self.n_points, self.n_no_normal = self.ctx.tsdf_extract_surface(1 if min_weight is None else min_weight)
        self.ctx.tsdf_surface_to_target()
        return self.n_points

    def _ray_params(self, shape, z_near, z_far, step, min_weight):
        shape = self.shape if shape is None else shape
        if shape is None:
            raise ValueError("the image's (rows, cols) is not known: pass shape")
        return binding.tsdf_raycast_params(shape=shape, fx=self.fx, cx=self.cx, z_near=z_near, z_far=z_far,
                                           step=0.0 if step is None else step, min_weight=min_weight)

    def raycast(self, pose, shape=None, z_near=0.25, z_far=6.0, step=None, min_weight=1):
        """The surface visible from the camera-to-world pose (4, 4), one ray per pixel of a (rows, cols) image with the
        volume's intrinsics (shape default: the last integrated frame's).  step: metres of camera depth between samples
        (default trunc / 2).  Returns dict(points (3, rows, cols), normals (3, rows, cols), depth, intensity, n_hits,
        n_no_normal); depth > 0 marks the pixels that hold a hit."""
        n_hits, n_no_normal = self.ctx.tsdf_raycast(pose, self._ray_params(shape, z_near, z_far, step, min_weight))
        return dict(self.ctx.tsdf_get_raycast(), n_hits=n_hits, n_no_normal=n_no_normal)

    def raycast_to_target(self, pose, shape=None, z_near=0.25, z_far=6.0, step=None, min_weight=1):
        """raycast, and its hits become the context's target with their normals (and colours), in row-major pixel
        order: device to device.  Returns n_hits; raises IcpkError (E_EMPTY_TARGET, the target stays) without any."""
        n_hits, _ = self.ctx.tsdf_raycast(pose, self._ray_params(shape, z_near, z_far, step, min_weight))
        self.ctx.tsdf_raycast_to_target()
        return n_hits

    def mesh(self, min_weight=1):
        """The surface as a triangle mesh (marching tetrahedra over the cells whose eight voxels have weight >=
        min_weight): dict(vertices (3, n), normals (3, n), intensity, voxel_index, edge, triangles (m, 3) int32,
        n_vertices, n_triangles, n_no_normal).  Vertices are ordered by owner voxel, then edge type; a vertex without a
        normal holds (0, 0, 0) and is counted in n_no_normal.  color: whether the intensities mean anything."""
        self.ctx.tsdf_extract_mesh(min_weight)
        return dict(self.ctx.tsdf_get_mesh(), color=bool(self.params.flags & binding.TSDF_COLOR))

    def set_planes(self, tsdf, weight, intensity=None):
        """The counterpart of planes(): a saved model, or an analytic field, becomes the volume's content."""
        self.ctx.tsdf_set(tsdf, weight, intensity)
        self.n_points = self.n_no_normal = None

    def planes(self, intensity=False):
        """(tsdf, weight, intensity) as (dz, dy, dx) arrays."""
        return self.ctx.tsdf_get(intensity=intensity)

    def box(self, lo, hi, intensity=False):
        """(tsdf, weight, intensity) of the sub-box lo <= (x, y, z) < hi, as (nz, ny, nx) arrays: what a caller who
        stitches a larger model offline archives of a slab before it leaves."""
        return binding.tsdf_get_box(self.ctx, lo, hi, intensity=intensity)

    def esdf(self, max_distance=2.0, min_weight=1, unknown_occupied=False, counts=True):
        """The exact Euclidean distance map of the volume as it stands (K31): per voxel the signed squared distance, in
        voxels, to the nearest voxel of the other kind -- occupied (weight >= min_weight and tsdf < 0; with
        unknown_occupied also every voxel below min_weight) against the rest --, exact up to max_distance metres and
        binding.ESDF_FAR beyond.  The map stays on the device, a snapshot: integrating further frames leaves it as it
        was (stale), and set_planes, shift, reset and release drop it.  Returns dict(unknown, free, occupied, far), the
        voxel counts, or None with counts=False (no host wait)."""
        n = binding.esdf_compute(self.ctx, max_distance=max_distance, min_weight=min_weight,
                                  flags=binding.ESDF_UNKNOWN_OCCUPIED if unknown_occupied else 0, counts=counts)
        return None if n is None else dict(unknown=int(n[0]), free=int(n[1]), occupied=int(n[2]), far=int(n[3]))

    def esdf_planes(self):
        """(sq int32, cls uint8, dist float32) of the last esdf(), as (dz, dy, dx) arrays: the signed squared distance,
        the class (0 unknown, 1 free, 2 occupied) and the metric distance in metres, positive outside the obstacles and
        zero half a voxel from an occupied voxel's centre."""
        return binding.esdf_get(self.ctx)

    def esdf_box(self, lo, hi):
        """esdf_planes() of the sub-box lo <= (x, y, z) < hi, as (nz, ny, nx) arrays."""
        return binding.esdf_get_box(self.ctx, lo, hi)

    def esdf_query(self, points):
        """The distance map at the world points (3, n), trilinear between voxel centres: dict(dist (n,) metres, grad
        (3, n): the gradient of that interpolant, pointing away from the obstacles, status (n,) uint8:
        binding.ESDF_Q_OUTSIDE for a point outside the centres' box (dist and grad 0), else ESDF_Q_FAR and
        ESDF_Q_UNKNOWN where a corner of the cell is beyond max_distance or of unknown class)."""
        return binding.esdf_query(self.ctx, points)

    def shift(self, s, min_weight=None):
        """The volume moves by s = (s_x, s_y, s_z) whole voxels (K23): the new voxel v holds the old voxel v + s, what
        falls off is gone and what comes in is fresh; the origin follows.  min_weight: first extract and download the
        leaving list -- the crossings the shift loses -- and return it as surface() does (else None)."""
        left = None
        if min_weight is not None:
            binding.tsdf_extract_leaving(self.ctx, s, min_weight)
            left = self.ctx.tsdf_get_surface()
        binding.tsdf_shift(self.ctx, s)
        self.params, self.total = binding.tsdf_get_params(self.ctx)
        self.n_points = self.n_no_normal = None
        return left

    @staticmethod
    def follow_steps(centre, ref, voxel):
        """k_a = round((c_a - ref_a) / voxel) in float64, halves away from zero: the whole voxels the camera centre
        has moved from the reference."""
        q = (np.asarray(centre, np.float64) - np.asarray(ref, np.float64)) / np.float64(voxel)
        return (np.sign(q) * np.floor(np.abs(q) + 0.5)).astype(np.int64)

    def follow(self, pose, every):
        """Keeps the volume around the camera: the first pose seen sets a reference centre; once the centre of `pose`
        (4, 4, camera-to-world) is `every` voxels or more from it along any axis, the volume shifts by the whole voxels
        k it has moved (all three axes) and the reference advances by k * voxel.  Returns the leaving list of that shift
        (extracted with self.follow_min_weight), or None when the volume stayed."""
        c = np.asarray(pose, np.float64).reshape(4, 4)[:3, 3]
        if self.follow_ref is None:
            self.follow_ref = c.copy()
        voxel = np.float64(self.params.voxel)
        k = self.follow_steps(c, self.follow_ref, voxel)
        if not (np.abs(k) >= int(every)).any():
            return None
        left = self.shift(k, min_weight=self.follow_min_weight)
        self.follow_ref = self.follow_ref + k.astype(np.float64) * voxel
        return left

    def reset(self):
        self.ctx.tsdf_reset()
        if self.total.any():  # (the box is back where it was created)
            self.params, self.total = binding.tsdf_get_params(self.ctx)
        self.follow_ref = None
        self.frames = 0
        self.n_points = self.n_no_normal = None

    def release(self):
        self.ctx.tsdf_release()


# K27's lost test: the defaults of ModelTracker(relocalise=...)'s min_overlap (pairs of level 0's last evaluated iteration
# over the frame's valid pixels) and max_mean_dist (their mean distance, metres).  Both are OFF: on the room arc the
# tracked frames and the wrong starts overlap in either quantity (DESIGN.md K27 holds the two tables: overlap 0.405 ..
# 0.772 tracked against 0.035 .. 0.682 from wrong starts, mean_dist 8.5 .. 11.9 mm against 9.9 .. 30.3 mm), so neither
# separates them and the test rests on level 0's status.
RELOCALISE_MIN_OVERLAP = 0.0
RELOCALISE_MAX_MEAN_DIST = float("inf")


class ModelTracker:
    """Frame-to-model tracking over a TsdfVolume: every frame is aligned point-to-plane against the model ray-cast at
    the last pose, then fused into the model at the pose found.  pose: the first frame's camera-to-world pose; z_near,
    z_far, step, min_weight: the ray cast's; align_kw: fields of icpk_params for the alignment (max_iterations,
    max_nn_dist, min_pairs, ...).  Keep max_nn_dist at a voxel or two: the target is the model seen from the LAST pose,
    so surfaces the new frame sees for the first time have no counterpart in it, and a wide gate pairs them with the
    view's border, which biases the pose (icpk_params' default, 0.75 m, is meant for frame-to-frame clouds).
    bilateral: a depth.bilateral_params object (True: the defaults) -- the cloud that is aligned then comes from the
    smoothed frame (depth.backproject_smoothed, K22) while the RAW frame is what the volume fuses, KinectFusion's order;
    None: the raw frame serves both.
    follow: an integer `every` -- the volume follows the camera (TsdfVolume.follow, K23): once a pose is found and before
    its frame is fused, the volume shifts when the camera has moved `every` voxels or more, and a non-empty leaving list
    goes to on_leave(list) (default: appended to self.streamed).  None: the volume stays where it was created.
    pyramid: a tuple of iteration counts, finest level first -- coarse-to-fine tracking over a depth pyramid (K24):
    (10, 5, 4) runs 4 iterations at level 2, then 5 at level 1, then 10 at level 0, each level against the model
    ray-cast at the LAST pose through (fx / 2^l, cx / 2^l) and through a gate of max_nn_dist * 2^l, since a pixel's
    footprint doubles per level; align_kw's max_iterations is not used then.  A level whose ray cast hits fewer pixels
    than min_pairs is skipped and counted in self.levels_skipped; only level 0 raises.  pyramid_cutoff: the rule's K
    (default: icpk_default_pyramid_params').  With bilateral, level 0 is the smoothed frame.  None: one alignment on
    the full frame.
    projective: True, or a dict of icpk_projective_params fields (max_dist, min_pairs, min_normal_cos) -- projective data
    association (K25) in place of the cloud-to-cloud alignment: the frame goes into a pyramid of len(pyramid) levels (1
    when pyramid is None; smoothed when bilateral is given), and per level, coarse to fine, the model is ray-cast at
    the LAST pose at the level's shape and intrinsics and binding.align_projective refines the estimate with
    pyramid[l] iterations (align_kw's max_iterations when pyramid is None).  No target list, no cloud, no index.  The
    gate max_dist is the SAME at every level and defaults to 0.5 m: a projective pair is as far apart as the frame has
    slid along a surface, so the gate must be wider than the frame's displacement (a tight one makes the first step
    nearly degenerate).  levels_skipped, level_hits and the level-0 RuntimeError are as above; level_stats holds
    ProjectiveResult objects.  None: the paths above, untouched.
    projective_color: True, or dict(lambda_geometric=, gradient_radius=, min_neighbors=) -- the photometric term beside
    the projective pairs (K26); it needs `projective` and a colour volume (ValueError otherwise), and track needs the
    frame's intensity.  Per frame the intensity goes beside the pyramid (never smoothed); per level, after the ray cast,
    binding.raycast_color_gradients (radius gradient_radius * 2^l, default 2 voxels at level 0; min_neighbors 4) and
    binding.align_projective_colored.  None: the projective path above, untouched.
    relocalise: True, or dict(fern= (a dict of FernParams fields; level defaults to the coarsest pyramid level), k= (3),
    min_overlap=, max_mean_dist=) -- fern keyframe relocalisation (K27); it needs `projective` (ValueError otherwise).
    A frame's alignment is accepted iff level 0's status is ICPK_OK, its count >= min_overlap * (the frame's valid
    pixels) and its mean_dist <= max_mean_dist.  An accepted frame is fused as above and goes through
    binding.fern_process(ctx, pose): keyframes are harvested from frames the tracker believes, the first frame included.  A
    frame that fails -- a level-0 ray cast below min_pairs included, which raises without relocalise -- is not fused,
    leaves the pose alone and sets self.lost.  While lost, a frame goes to the relocaliser first: its k nearest keyframes
    (none when the frame has fewer than min_valid valid ferns) are tried in order, each as both the ray casts' pose and
    the start of the same coarse-to-fine loop, and the first that passes the test becomes the pose; the frame is fused
    and lost is cleared.  track returns the pose either way: callers read self.lost, and self.relocalisations,
    self.frames_lost, self.keyframes count.  None: every path above, untouched.
    sdf: True, or dict(max_abs_tsdf=, min_pairs=, min_normal_cos=) -- the frame is aligned directly against the distance
    field (K29), with no ray cast at any level: the frame goes into a pyramid of len(pyramid) levels (1 when pyramid is
    None; smoothed when bilateral is given), and per level, coarse to fine, binding.align_sdf runs pyramid[l] iterations
    (align_kw's max_iterations when pyramid is None) from the estimate so far, through the tracker's min_weight.  The
    frame is then fused as before; `follow` works, because the rule reads the volume's current origin.  level_stats
    holds the ProjectiveResult objects; n_hits and level_hits stay None.  Together with projective, projective_color or
    relocalise it raises ValueError.  None: every path above, untouched."""

    def __init__(self, vol, pose=None, z_near=0.25, z_far=6.0, step=None, min_weight=1, bilateral=None, follow=None,
                 on_leave=None, pyramid=None, pyramid_cutoff=None, projective=None, projective_color=None, relocalise=None,
                 sdf=None, **align_kw):
        if sdf is not None:  # (K29: said before anything the other settings have to say)
            for name, other in (("projective", projective), ("projective_color", projective_color), ("relocalise", relocalise)):
                if other is not None:
                    raise ValueError(f"sdf does not go together with {name}")
        self.vol = vol
        self.pose = np.eye(4) if pose is None else np.array(pose, np.float64).reshape(4, 4)
        self.ray = dict(z_near=z_near, z_far=z_far, step=step, min_weight=min_weight)
        self.align_kw = align_kw
        self.bilateral = depth_front.bilateral_params() if bilateral is True else bilateral
        self.frames = 0
        self.n_hits = self.stats = None
        self.follow = follow
        self.streamed = []
        self.on_leave = self.streamed.append if on_leave is None else on_leave
        self.shifts = 0  # the shifts `follow` has made
        self.pyramid = None if pyramid is None else tuple(int(n) for n in pyramid)
        if self.pyramid is not None and not 1 <= len(self.pyramid) <= binding.PYRAMID_MAX_LEVELS:
            raise ValueError(f"pyramid: 1 .. {binding.PYRAMID_MAX_LEVELS} iteration counts, finest level first")
        self.pyramid_params = None
        if self.pyramid is not None:
            kw = {} if pyramid_cutoff is None else dict(range_cutoff=int(pyramid_cutoff))
            self.pyramid_params = depth_front.pyramid_params(levels=len(self.pyramid), **kw)
        self.levels_skipped = 0  # pyramid levels whose ray cast hit fewer pixels than min_pairs
        self.level_hits = self.level_stats = None  # per level of the last frame, finest first (None: skipped)
        self.projective = None if projective is None else ({} if projective is True else dict(projective))
        if self.projective is not None:
            self.projective.setdefault("max_dist", 0.5)
            if "min_pairs" in align_kw:
                self.projective.setdefault("min_pairs", align_kw["min_pairs"])
            self.projective_counts = self.pyramid if self.pyramid is not None else \
                (int(align_kw.get("max_iterations", binding.default_projective_params().max_iterations)),)
            if self.pyramid_params is None:
                kw = {} if pyramid_cutoff is None else dict(range_cutoff=int(pyramid_cutoff))
                self.pyramid_params = depth_front.pyramid_params(levels=1, **kw)
        # K26: the photometric term beside the projective pairs -- None, True or dict(lambda_geometric=, gradient_radius=
        # (at level 0; level l takes 2^l times it; default 2 voxels), min_neighbors= (4))
        self.projective_color = None if projective_color is None else ({} if projective_color is True else dict(projective_color))
        if self.projective_color is not None:
            if self.projective is None:
                raise ValueError("projective_color needs projective")
            if not vol.params.flags & binding.TSDF_COLOR:
                raise ValueError("projective_color needs a colour volume")
            unknown = set(self.projective_color) - {"lambda_geometric", "gradient_radius", "min_neighbors"}
            if unknown:
                raise ValueError(f"projective_color has no setting {sorted(unknown)}")
        # K27: None, True or dict(fern= (FernParams fields; level: the coarsest pyramid level), k= (3), min_overlap=,
        # max_mean_dist=)
        self.relocalise = None if relocalise is None else ({} if relocalise is True else dict(relocalise))
        self.lost = False
        self.relocalisations = self.frames_lost = 0
        self._reloc = None  # the depth.Relocaliser, made with the first frame (its level's shape is the frame's)
        if self.relocalise is not None:
            if self.projective is None:
                raise ValueError("relocalise needs projective")
            unknown = set(self.relocalise) - {"fern", "k", "min_overlap", "max_mean_dist"}
            if unknown:
                raise ValueError(f"relocalise has no setting {sorted(unknown)}")
            self.relocalise_k = int(self.relocalise.get("k", 3))
            if not 1 <= self.relocalise_k <= binding.FERN_MAX_K:
                raise ValueError(f"relocalise: k in 1 .. {binding.FERN_MAX_K}")
            self.min_overlap = float(self.relocalise.get("min_overlap", RELOCALISE_MIN_OVERLAP))
            self.max_mean_dist = float(self.relocalise.get("max_mean_dist", RELOCALISE_MAX_MEAN_DIST))
        # K29: None, True or dict(max_abs_tsdf=, min_pairs=, min_normal_cos=)
        self.sdf = None if sdf is None else ({} if sdf is True else dict(sdf))
        if self.sdf is not None:
            unknown = set(self.sdf) - {"max_abs_tsdf", "min_pairs", "min_normal_cos"}
            if unknown:
                raise ValueError(f"sdf has no setting {sorted(unknown)}")
            if "min_pairs" in align_kw:
                self.sdf.setdefault("min_pairs", align_kw["min_pairs"])
            self.sdf_counts = self.pyramid if self.pyramid is not None else \
                (int(align_kw.get("max_iterations", binding.default_sdf_params().max_iterations)),)
            if self.pyramid_params is None:
                kw = {} if pyramid_cutoff is None else dict(range_cutoff=int(pyramid_cutoff))
                self.pyramid_params = depth_front.pyramid_params(levels=1, **kw)

    def _track_sdf(self, depth):
        """The pose of one frame against the distance field itself, coarse to fine: one build, then per level the device
        loop over the level and the volume's planes, both where they lie.  No ray cast."""
        vol, ctx = self.vol, self.vol.ctx
        shapes = depth_front.build_pyramid(ctx, depth, self.pyramid_params, smooth=self.bilateral)
        estimate = self.pose
        self.level_hits, self.level_stats = None, [None] * len(shapes)
        for l in range(len(shapes) - 1, -1, -1):
            params = binding.default_sdf_params(**dict(self.sdf, level=l, fx=vol.fx, cx=vol.cx, max_iterations=self.sdf_counts[l],
                                                       min_weight=self.ray["min_weight"]))
            estimate, self.level_stats[l] = binding.align_sdf(ctx, estimate, params)
        self.n_hits, self.stats = None, self.level_stats[0]
        return estimate

    def _track_projective(self, depth, intensity=None):
        """The pose of one frame by projective association, coarse to fine: one build, then per level a ray cast of the
        model at the last pose and the device loop over the level and the maps, both where they lie."""
        # (with `bilateral` the depth is smoothed and the intensity is not)
        shapes = depth_front.build_pyramid(self.vol.ctx, depth, self.pyramid_params, smooth=self.bilateral,
                                           intensity=None if self.projective_color is None else intensity)
        return self._projective_levels(shapes, self.pose)

    def _projective_levels(self, shapes, pose, soft=False):
        """The coarse-to-fine loop over the resident pyramid: `pose` is both the ray casts' pose and the start.  soft
        (K27): a level-0 ray cast below min_pairs returns None in place of raising."""
        vol, ctx = self.vol, self.vol.ctx
        color = self.projective_color
        if color is not None:
            cparams = binding.default_projective_color_params(**{k: color[k] for k in ("lambda_geometric",) if k in color})
            radius0 = float(color.get("gradient_radius", 2.0 * vol.params.voxel))
        estimate = pose
        self.level_hits, self.level_stats = [None] * len(shapes), [None] * len(shapes)
        for l in range(len(shapes) - 1, -1, -1):
            scale = float(2 ** l)
            params = binding.default_projective_params(**dict(self.projective, level=l, fx=vol.fx, cx=vol.cx,
                                                              max_iterations=self.projective_counts[l]))
            ray = binding.tsdf_raycast_params(shape=shapes[l], fx=vol.fx / scale, cx=vol.cx / scale, z_near=self.ray["z_near"],
                                              z_far=self.ray["z_far"], step=0.0 if self.ray["step"] is None else self.ray["step"],
                                              min_weight=self.ray["min_weight"])
            n_hits, _ = ctx.tsdf_raycast(pose, ray)
            self.level_hits[l] = n_hits
            if n_hits < params.min_pairs:
                if l == 0:
                    if soft:
                        self.n_hits, self.stats = n_hits, None
                        return None
                    raise RuntimeError(f"the ray cast hit the model in {n_hits} pixels, fewer than min_pairs = {params.min_pairs}")
                self.levels_skipped += 1
                continue
            if color is None:
                estimate, self.level_stats[l] = binding.align_projective(ctx, estimate, params)
            else:
                binding.raycast_color_gradients(ctx, radius0 * scale, int(color.get("min_neighbors", 4)))
                estimate, self.level_stats[l] = binding.align_projective_colored(ctx, estimate, params, cparams)
        self.n_hits, self.stats = self.level_hits[0], self.level_stats[0]
        return estimate

    # ---- K27: the lost test and the way back ----
    def accepted(self, valid):
        """The lost test on the last alignment: level 0's status is ICPK_OK, its pairs are at least min_overlap of the
        frame's `valid` pixels, and their mean distance is at most max_mean_dist."""
        st = self.stats
        return st is not None and st.status == binding.OK and st.count >= self.min_overlap * valid and \
            st.mean_dist <= self.max_mean_dist

    @property
    def keyframes(self):
        return 0 if self._reloc is None else self._reloc.count

    def _fuse(self, depth, intensity):
        vol = self.vol
        if self.follow is not None:
            before = vol.total.copy()
            left = vol.follow(self.pose, self.follow)
            self.shifts += bool((vol.total != before).any())
            if left is not None and left["points"].shape[1] > 0:
                self.on_leave(left)
        vol.integrate(depth, self.pose, intensity)
        self.frames += 1

    def _track_relocalise(self, depth, intensity):
        """track() with relocalise: a frame whose alignment fails the lost test is not fused and leaves the pose alone;
        while lost, a frame is looked up among the keyframes and the alignment restarts from their poses."""
        ctx = self.vol.ctx
        shapes = depth_front.build_pyramid(ctx, depth, self.pyramid_params, smooth=self.bilateral,
                                           intensity=None if self.projective_color is None else intensity)
        if self._reloc is None:
            fern = dict(self.relocalise.get("fern", {}))
            fern.setdefault("level", len(shapes) - 1)
            self._reloc = depth_front.Relocaliser(ctx, shapes[fern["level"]] if 0 <= fern["level"] < len(shapes) else (0, 0),
                                                  **fern)
        if self.frames > 0:
            valid = int(np.count_nonzero(depth))
            found = None
            if not self.lost:
                estimate = self._projective_levels(shapes, self.pose, soft=True)
                if estimate is not None and self.accepted(valid):
                    found = estimate
            else:
                r = self._reloc.process(None, self.relocalise_k)
                if r["valid"] >= self._reloc.params.min_valid:  # (a frame with too few valid ferns is not tried)
                    for candidate in r["poses"]:
                        estimate = self._projective_levels(shapes, candidate, soft=True)
                        if estimate is not None and self.accepted(valid):
                            found = estimate
                            self.relocalisations += 1
                            break
            if found is None:
                self.lost = True
                self.frames_lost += 1
                return self.pose.copy()
            self.lost = False
            self.pose = found
        self._fuse(depth, intensity)
        self._reloc.process(self.pose, 1)  # keyframes come from frames the tracker believes, the first one included
        return self.pose.copy()

    def _track_pyramid(self, depth):
        """The pose of one frame, coarse to fine: one build, then per level a ray cast of the model at the last pose,
        the level's cloud moved by the running estimate, and an alignment that refines the estimate."""
        vol, ctx = self.vol, self.vol.ctx
        shapes = depth_front.build_pyramid(ctx, depth, self.pyramid_params, smooth=self.bilateral)
        gate = binding.default_params(**self.align_kw).max_nn_dist
        estimate = self.pose
        self.level_hits, self.level_stats = [None] * len(shapes), [None] * len(shapes)
        for l in range(len(shapes) - 1, -1, -1):
            scale = float(2 ** l)
            params = binding.default_params(**dict(self.align_kw, solve=binding.SOLVE_POINT_TO_PLANE,
                                                   max_iterations=self.pyramid[l], max_nn_dist=gate * scale))
            ray = binding.tsdf_raycast_params(shape=shapes[l], fx=vol.fx / scale, cx=vol.cx / scale, z_near=self.ray["z_near"],
                                              z_far=self.ray["z_far"], step=0.0 if self.ray["step"] is None else self.ray["step"],
                                              min_weight=self.ray["min_weight"])
            n_hits, _ = ctx.tsdf_raycast(self.pose, ray)
            self.level_hits[l] = n_hits
            if n_hits < params.min_pairs:
                if l == 0:
                    raise RuntimeError(f"the ray cast hit the model in {n_hits} pixels, fewer than min_pairs = {params.min_pairs}")
                self.levels_skipped += 1
                continue
            ctx.tsdf_raycast_to_target()
            depth_front.backproject_level(ctx, l, which=0, fx=vol.fx, cx=vol.cx)
            ctx.transform_source(estimate[:3, :3], estimate[:3, 3])
            ctx.commit_source()
            T, self.level_stats[l], _ = ctx.align(params)
            estimate = T.astype(np.float64) @ estimate
        self.n_hits, self.stats = self.level_hits[0], self.level_stats[0]
        return estimate

    def track(self, depth, intensity=None):
        """One (rows, cols) uint16 frame (with its (rows, cols) intensities on a colour volume).  Returns the frame's
        camera-to-world pose (4, 4) float64; the first frame takes the initial pose."""
        vol, ctx = self.vol, self.vol.ctx
        if self.projective_color is not None and intensity is None:
            raise ValueError("projective_color needs the frame's intensity")
        if self.relocalise is not None:
            return self._track_relocalise(depth, intensity)
        if self.frames > 0 and self.sdf is not None:
            self.pose = self._track_sdf(depth)
        elif self.frames > 0 and self.projective is not None:
            self.pose = self._track_projective(depth, intensity)
        elif self.frames > 0 and self.pyramid is not None:
            self.pose = self._track_pyramid(depth)
        elif self.frames > 0:
            params = binding.default_params(solve=binding.SOLVE_POINT_TO_PLANE, **self.align_kw)
            self.n_hits, _ = ctx.tsdf_raycast(self.pose, vol._ray_params(np.shape(depth), **self.ray))
            if self.n_hits < params.min_pairs:
                raise RuntimeError(f"the ray cast hit the model in {self.n_hits} pixels, fewer than min_pairs = {params.min_pairs}")
            ctx.tsdf_raycast_to_target()
            if self.bilateral is None:
                ctx.backproject(depth, which=0, fx=vol.fx, cx=vol.cx)
            else:
                depth_front.backproject_smoothed(ctx, depth, which=0, fx=vol.fx, cx=vol.cx, params=self.bilateral)
            ctx.transform_source(self.pose[:3, :3], self.pose[:3, 3])
            ctx.commit_source()
            T, self.stats, _ = ctx.align(params)
            self.pose = T.astype(np.float64) @ self.pose
        self._fuse(depth, intensity)
        return self.pose.copy()


_PLY_TYPES = {"float": "<f4", "float32": "<f4", "int": "<i4", "int32": "<i4", "uchar": "u1", "uint8": "u1"}


def write_ply(path, mesh, color=None):
    """A mesh of TsdfVolume.mesh as binary little-endian PLY: per vertex x, y, z, nx, ny, nz (and `intensity`, a float
    scalar, when the mesh comes from a colour volume; color overrides mesh["color"]), per face a list of three int32
    vertex indices."""
    color = bool(mesh.get("color", False)) if color is None else bool(color)
    v, nrm = np.asarray(mesh["vertices"], "<f4"), np.asarray(mesh["normals"], "<f4")
    tri = np.asarray(mesh["triangles"], "<i4").reshape(-1, 3)
    names = ["x", "y", "z", "nx", "ny", "nz"] + (["intensity"] if color else [])
    vert = np.empty(v.shape[1], [(k, "<f4") for k in names])
    for k in range(3):
        vert[names[k]], vert[names[3 + k]] = v[k], nrm[k]
    if color:
        vert["intensity"] = np.asarray(mesh["intensity"], "<f4")
    face = np.empty(tri.shape[0], [("n", "u1"), ("i", "<i4", (3,))])
    face["n"], face["i"] = 3, tri
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {vert.size}"] + \
        [f"property float {k}" for k in names] + [f"element face {face.size}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vert.tobytes())
        fh.write(face.tobytes())


def read_ply(path):
    """What write_ply wrote (binary little-endian, float vertex properties, triangles only), back as dict(vertices (3, n),
    normals (3, n), intensity, triangles (m, 3), color)."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError("not a binary little-endian PLY file")
    nvert = nface = 0
    props, element = [], None
    for ln in lines[2:]:
        w = ln.split()
        if w[:1] == ["element"]:
            element = w[1]
            if element == "vertex":
                nvert = int(w[2])
            elif element == "face":
                nface = int(w[2])
        elif w[:1] == ["property"] and element == "vertex":
            props.append((w[2], _PLY_TYPES[w[1]]))
        elif w[:1] == ["property"] and element == "face" and w[1:4] != ["list", "uchar", "int"]:
            raise ValueError("faces must be lists of uchar counts and int indices")
    vert = np.frombuffer(data, np.dtype(props), nvert, end)
    face = np.frombuffer(data, np.dtype([("n", "u1"), ("i", "<i4", (3,))]), nface, end + vert.nbytes)
    if nface and not np.all(face["n"] == 3):
        raise ValueError("only triangles are read")
    color = "intensity" in vert.dtype.names
    f32 = np.float32
    return dict(vertices=np.stack([vert[k] for k in "xyz"]).astype(f32), normals=np.stack([vert[k] for k in ("nx", "ny", "nz")]).astype(f32),
                intensity=vert["intensity"].astype(f32) if color else np.zeros(nvert, f32),
                triangles=face["i"].astype(np.int32).reshape(-1, 3), color=color)
