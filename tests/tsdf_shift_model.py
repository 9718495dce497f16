"""numpy restatement of the shift rule and the leaving list of the TSDF volume (K23, include/icpk.h) on top of
tests/tsdf_model.py: the planes moved by whole voxels, the origin always from the creation origin and the cumulative
shift, and the surface list filtered by the stencil predicate."""
import numpy as np

import tsdf_model

F = np.float32


def origin_after(origin0, total, voxel):
    """origin_a = (float)((double)origin0_a + (double)total_a * (double)voxel)"""
    return (np.asarray(origin0, F).astype(np.float64) + np.asarray(total, np.int64).astype(np.float64) * np.float64(F(voxel))).astype(F)


def _moved(plane, s, dims):
    """new[k, j, i] = old[k + s_z, j + s_y, i + s_x] where that is in bounds, else 0"""
    out = np.zeros_like(plane)
    src, dst = [], []
    for a in (2, 1, 0):  # (the planes are (dz, dy, dx))
        n, sa = dims[a], int(s[a])
        lo, hi = max(0, -sa), min(n, n - sa)  # destination indices whose source lo + sa .. hi + sa is in bounds
        if lo >= hi:
            return out
        dst.append(slice(lo, hi))
        src.append(slice(lo + sa, hi + sa))
    out[tuple(dst)] = plane[tuple(src)]
    return out


def shifted(vol, s):
    """The tsdf_model.Volume after icpk_tsdf_shift(s): moved planes, the origin by the rule.  The creation origin and the
    cumulative shift ride along as .origin0 and .total (a Volume that was never shifted has its own origin and zero)."""
    s = [int(x) for x in s]
    out = tsdf_model.Volume(vol.dims, vol.voxel, vol.origin, vol.trunc, max_weight=vol.max_weight,
                            depth_scale=vol.depth_scale, color=vol.intensity is not None)
    out.origin0 = np.array(getattr(vol, "origin0", vol.origin), F)
    out.total = np.asarray(getattr(vol, "total", np.zeros(3, np.int64)), np.int64) + np.asarray(s, np.int64)
    out.origin = origin_after(out.origin0, out.total, vol.voxel)
    out.tsdf = _moved(vol.tsdf, s, vol.dims)
    out.weight = _moved(vol.weight, s, vol.dims)
    if vol.intensity is not None:
        out.intensity = _moved(vol.intensity, s, vol.dims)
    return out


def _coords(voxel, dims):
    v = np.asarray(voxel, np.int64)
    return [v % dims[0], (v // dims[0]) % dims[1], v // (dims[0] * dims[1])]


def kept_mask(voxel, axis, s, dims):
    """A crossing (V, N = V + 1 along axis) is kept iff V, N and the six axis neighbours of each stay, stays(v): s_a <=
    v_a < dims_a + s_a"""
    c = _coords(voxel, dims)
    keep = np.ones(len(c[0]), bool)
    for a in range(3):
        lo, hi = int(s[a]), dims[a] + int(s[a])
        keep &= (c[a] - 1 >= lo) & (c[a] + 1 + (np.asarray(axis) == a) < hi)
    return keep


def ends_stay_mask(voxel, axis, s, dims):
    c = _coords(voxel, dims)
    stay = np.ones(len(c[0]), bool)
    for a in range(3):
        lo, hi = int(s[a]), dims[a] + int(s[a])
        stay &= (c[a] >= lo) & (c[a] + (np.asarray(axis) == a) < hi)
    return stay


def leaving(vol, s, min_weight=1, surface=None):
    """icpk_tsdf_extract_leaving: dict(points, normals, intensity, voxel, axis, n_no_normal, kept) -- the crossings of
    vol.extract(min_weight) (or of `surface`, that very list computed earlier) the shift does not keep, in its order;
    n_no_normal: the dropped crossings one of whose ends does not stay; kept: the mask over the full list."""
    e = vol.extract(min_weight) if surface is None else surface
    kept = kept_mask(e["voxel"], e["axis"], s, vol.dims)
    gone = ~kept
    lost = ~ends_stay_mask(e["dropped_voxel"], e["dropped_axis"], s, vol.dims)
    return dict(points=e["points"][:, gone], normals=e["normals"][:, gone], intensity=e["intensity"][gone],
                voxel=e["voxel"][gone], axis=e["axis"][gone], n_no_normal=int(lost.sum()), kept=kept)


def map_back(voxel, s, dims):
    """the old linear index of the voxels of a shifted volume"""
    c = _coords(voxel, dims)
    return (c[0] + int(s[0])) + dims[0] * ((c[1] + int(s[1])) + dims[1] * (c[2] + int(s[2])))


def follow_steps(centre, ref, voxel):
    """TsdfVolume.follow's k, written independently: round half away from zero of (c - ref) / voxel in float64"""
    out = []
    for c, r in zip(np.asarray(centre, np.float64), np.asarray(ref, np.float64)):
        q = (c - r) / np.float64(voxel)
        out.append(int(np.floor(q + 0.5)) if q >= 0 else -int(np.floor(-q + 0.5)))
    return np.array(out, np.int64)
