"""The model the poses are for (K19): a dense volume of truncated signed distances on the device, into which posed
depth frames are fused (Context.tsdf_integrate) and from which the surface comes back as points with normals
(Context.tsdf_extract_surface) -- or goes on to be the context's target for scan-to-model alignment.

    vol = TsdfVolume(ctx, dims=(256, 256, 256), voxel=0.02, origin=(-2.56, -2.56, 0.0), trunc=0.08)
    vol.integrate_all(depths, graph.poses())   # the optimised poses of posegraph.PoseGraph, camera-to-world
    model = vol.surface(min_weight=2)          # dict(points, normals, intensity, voxel, axis)
    vol.to_target()                            # ... or: the next frame is aligned against the model
"""
import numpy as np

from . import binding


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

    def planes(self, intensity=False):
        """(tsdf, weight, intensity) as (dz, dy, dx) arrays."""
        return self.ctx.tsdf_get(intensity=intensity)

    def reset(self):
        self.ctx.tsdf_reset()
        self.frames = 0
        self.n_points = self.n_no_normal = None

    def release(self):
        self.ctx.tsdf_release()
