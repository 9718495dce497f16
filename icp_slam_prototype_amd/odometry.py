"""Projective frame-to-frame odometry (K28): the projective loop (K25, coloured K26) against a view built from a depth
frame alone -- the previous frame's, or a keyframe's, vertex and normal map (binding.frame_view_build) -- instead of the
ray cast of a TSDF volume.  No volume is created, fused or cast."""
import numpy as np

from . import binding
from . import depth as depth_front


def _motion(a, b):
    """(degrees, metres) from pose a to pose b"""
    E = np.linalg.inv(a) @ b
    return float(np.degrees(np.arccos(np.clip((np.trace(E[:3, :3]) - 1) / 2, -1, 1)))), float(np.linalg.norm(E[:3, 3]))


class ProjectiveOdometry:
    """Poses of a depth (or RGB-D) stream by projective alignment of every frame to a frame view.

        odo = ProjectiveOdometry(ctx, pose=first_pose, fx=fx, cx=cx)
        for frame in frames:
            pose = odo.track(frame)         # the frame's pyramid is resident afterwards, so
            reloc.process(pose)             # a depth.Relocaliser of the same context reads it beside the odometry

    pyramid: the iteration counts per level, finest first (its length is the number of levels).
    projective: None / True, or a dict of ProjectiveParams fields (max_dist, min_normal_cos, min_pairs).
    color: None, True, or dict(lambda_geometric=, gradient_radius= (metres at level 0; level l takes 2^l times it;
        default 0.1), min_neighbors= (4)) -- the photometric term; track then needs the frame's intensity.
    bilateral: a depth.bilateral_params object or True -- level 0 is smoothed (the intensity never is).
    keyframe: None -- the view is rebuilt from every frame at the pose found (frame to frame) --, or
        dict(min_overlap=, max_angle_deg=, max_shift=): the view is kept, and rebuilt from the current frame only when the
        level-0 pair count falls below min_overlap of the frame's valid pixels or the pose has moved past a bound from the
        view's pose (frame to keyframe: no error accumulates between rebuilds).  A bound left out does not apply.

    Per frame, track(depth, intensity=None): depth.build_pyramid; the first frame takes `pose` and builds the view;
    every other frame runs, coarse to fine, binding.projective_set_view(ctx, VIEW_FRAME, l) and binding.align_projective (or
    align_projective_colored, after binding.frame_view_color_gradients once per level of a view), each level starting
    from the running estimate, the coarsest from the last pose.  A level whose view has fewer valid pixels than min_pairs
    is skipped and counted in levels_skipped; only level 0 raises.  The selector is put back to VIEW_RAYCAST before
    track returns.  level_stats (ProjectiveResult per level of the last frame, None: skipped), level_valid (the view's
    valid pixels per level), views_built, frames, pose and view_pose are there to be read."""

    def __init__(self, ctx, pose=None, pyramid=(10, 5, 4), projective=None, color=None, bilateral=None, keyframe=None,
                 fx=468.60, cx=318.27):
        self.ctx = ctx
        self.pose = np.eye(4) if pose is None else np.array(pose, np.float64).reshape(4, 4)
        self.counts = tuple(int(n) for n in pyramid)
        if not 1 <= len(self.counts) <= binding.PYRAMID_MAX_LEVELS:
            raise ValueError(f"pyramid: 1 .. {binding.PYRAMID_MAX_LEVELS} iteration counts, finest level first")
        self.pyramid_params = depth_front.pyramid_params(levels=len(self.counts))
        self.projective = {} if projective is None or projective is True else dict(projective)
        self.projective.setdefault("max_dist", 0.5)
        self.color = None if color is None else ({} if color is True else dict(color))
        if self.color is not None:
            unknown = set(self.color) - {"lambda_geometric", "gradient_radius", "min_neighbors"}
            if unknown:
                raise ValueError(f"color has no setting {sorted(unknown)}")
        self.bilateral = depth_front.bilateral_params() if bilateral is True else bilateral
        self.keyframe = None if keyframe is None else dict(keyframe)
        if self.keyframe is not None:
            unknown = set(self.keyframe) - {"min_overlap", "max_angle_deg", "max_shift"}
            if unknown:
                raise ValueError(f"keyframe has no setting {sorted(unknown)}")
        self.fx, self.cx = float(fx), float(cx)
        self.frames = self.views_built = self.levels_skipped = 0
        self.level_stats = self.level_valid = self.view_pose = None

    def _build_view(self):
        self.level_valid, _ = binding.frame_view_build(self.ctx, self.pose, fx=self.fx, cx=self.cx)
        self.view_pose = self.pose.copy()
        self.views_built += 1
        if self.color is not None:
            radius0 = float(self.color.get("gradient_radius", 0.1))
            for l in range(len(self.counts)):
                binding.frame_view_color_gradients(self.ctx, l, radius0 * 2 ** l, int(self.color.get("min_neighbors", 4)))

    def _align(self):
        ctx = self.ctx
        cparams = None
        if self.color is not None:
            cparams = binding.default_projective_color_params(**{k: self.color[k] for k in ("lambda_geometric",) if k in self.color})
        estimate = self.pose
        self.level_stats = [None] * len(self.counts)
        try:
            for l in range(len(self.counts) - 1, -1, -1):
                params = binding.default_projective_params(**dict(self.projective, level=l, fx=self.fx, cx=self.cx,
                                                                  max_iterations=self.counts[l]))
                if self.level_valid[l] < params.min_pairs:
                    if l == 0:
                        raise RuntimeError(f"the view has {self.level_valid[l]} valid pixels, fewer than min_pairs = {params.min_pairs}")
                    self.levels_skipped += 1
                    continue
                binding.projective_set_view(ctx, binding.VIEW_FRAME, l)
                if cparams is None:
                    estimate, self.level_stats[l] = binding.align_projective(ctx, estimate, params)
                else:
                    estimate, self.level_stats[l] = binding.align_projective_colored(ctx, estimate, params, cparams)
        finally:
            binding.projective_set_view(ctx, binding.VIEW_RAYCAST)
        return estimate

    def _view_is_spent(self, valid):
        k = self.keyframe
        if k is None:
            return True
        angle, shift = _motion(self.view_pose, self.pose)
        return ("min_overlap" in k and self.level_stats[0].count < k["min_overlap"] * valid) or \
            ("max_angle_deg" in k and angle > k["max_angle_deg"]) or ("max_shift" in k and shift > k["max_shift"])

    def track(self, depth, intensity=None):
        """One (rows, cols) uint16 frame (with its (rows, cols) float32 intensities when `color` is set).  Returns the
        frame's camera-to-world pose (4, 4) float64; the first frame takes the initial pose."""
        if self.color is not None and intensity is None:
            raise ValueError("color needs the frame's intensity")
        depth_front.build_pyramid(self.ctx, depth, self.pyramid_params, smooth=self.bilateral,
                                  intensity=None if self.color is None else intensity)
        if self.frames == 0:
            self._build_view()
        else:
            self.pose = self._align()
            if self._view_is_spent(int(np.count_nonzero(depth))):
                self._build_view()
        self.frames += 1
        return self.pose.copy()
