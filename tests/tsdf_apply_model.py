"""numpy restatement of the signed update rule of the TSDF volume (K30, include/icpk.h) over tests/tsdf_model.py: rules
1 - 7 are that model's (run on a scratch copy of the volume, so that nothing is restated twice), the +1 branch is its
rules 8 - 10 and the -1 branch is written here.  Elementwise float32, one rounding per operation in the header's order:
the device and icpk_tsdf_voxel_apply are held against it bit for bit.  Also the error bound of a removal, derived
below."""
import copy

import numpy as np

import tsdf_model

F = np.float32
EPS = 2.0 ** -24  # half an ulp of 1 in float32: the relative error of one rounding


def sample(vol, depth, pose, fx, cx, intensity=None):
    """Rules 1 - 7 for every voxel: (ok, f, c) -- whether the frame produces a sample there, the sample, and the pixel's
    intensity (None without colour).  The volume is not changed."""
    scratch = copy.copy(vol)
    scratch.tsdf, scratch.weight = vol.tsdf.copy(), vol.weight.copy()
    scratch.intensity = None
    depth = np.asarray(depth, np.uint16)
    _, dbg = scratch.integrate(depth, pose, fx, cx, debug=True)
    ok = dbg["ok"]
    with np.errstate(all="ignore"):
        f = np.minimum(F(1), dbg["sdf"] / vol.trunc)
        c = None
        if intensity is not None:
            col = np.where(ok, np.floor(dbg["u"] + F(0.5)), 0).astype(np.int64)
            row = np.where(ok, np.floor(dbg["v"] + F(0.5)), 0).astype(np.int64)
            c = np.asarray(intensity, F).reshape(depth.shape)[row, col]
    return ok, f.astype(F), c


def _blend(value, wf, s):
    return ((value * wf) + s) / (wf + F(1))


def _unblend(value, wf, s, lo):
    with np.errstate(all="ignore"):
        r = ((value * wf) - s) / (wf - F(1))
    return np.minimum(np.maximum(r, F(lo)), F(1))


def apply(vol, frames, ops, fx, cx, intensities=None):
    """The ops -- (sign, frame, pose) -- on the tsdf_model.Volume in order; returns the voxels every op wrote."""
    counts = []
    color = vol.intensity is not None
    for sign, frame, pose in ops:
        ok, f, c = sample(vol, frames[frame], pose, fx, cx, intensities[frame] if color else None)
        w = vol.weight.astype(np.int64)
        wf = vol.weight.astype(F)
        if sign > 0:
            wrote = ok
            tsdf = _blend(vol.tsdf, wf, f)
            inten = _blend(vol.intensity, wf, c) if color else None
            neww = np.minimum(w + 1, vol.max_weight)
        else:
            wrote = ok & (w > 0)
            one = w == 1
            tsdf = np.where(one, F(0), _unblend(vol.tsdf, wf, f, -1))
            inten = np.where(one, F(0), _unblend(vol.intensity, wf, c, 0)) if color else None
            neww = w - 1
        vol.tsdf = np.where(wrote, tsdf, vol.tsdf).astype(F)
        if color:
            vol.intensity = np.where(wrote, inten, vol.intensity).astype(F)
        vol.weight = np.where(wrote, neww, w).astype(np.uint16)
        counts.append(int(wrote.sum()))
    return counts


def error_bound(signs):
    """A bound, in units of EPS, on |tsdf - the exact mean of the samples the voxel holds| after the ops `signs` have
    all hit one fresh, never saturated voxel (None where the sequence removes from an empty voxel).  e: the bound so
    far, w: the weight before the op; every sample and every exact mean lies in [-1, 1].
      +1  fl(fl(fl(m w) + f) / (w + 1)): the product carries w e and rounds by at most w EPS, the sum rounds by at most
          (w + 1) EPS, the quotient divides both by w + 1 and rounds by at most EPS:  e' = (w e + (2 w + 1)) / (w + 1) + 1,
          and e' = 0 for w = 0 (0 * 0 + f and f / 1 are exact).
      -1  fl(fl(fl(m w) - f) / (w - 1)): the same with the divisor w - 1:  e' = (w e + (2 w + 1)) / (w - 1) + 1; the clamp
          to [-1, 1] moves the value towards the exact mean; w = 1 gives the fresh state, e' = 0.
    The roundings are relative to magnitudes that exceed w, w + 1 and 1 by the error itself: a factor 1 + 2^-16 on the
    result covers that."""
    e, w = 0.0, 0
    for s in signs:
        if s > 0:
            e = 0.0 if w == 0 else (w * e + 2 * w + 1) / (w + 1) + 1
            w += 1
        else:
            if w == 0:
                return None
            e = 0.0 if w == 1 else (w * e + 2 * w + 1) / (w - 1) + 1
            w -= 1
    return e * (1 + 2.0 ** -16)


def any_subsequence_error_bound(signs):
    """error_bound's worst over EVERY subsequence of the ops, in units of EPS, for lists too long to enumerate by key: a
    sweep over the ops that keeps, per weight w, the largest bound a voxel with that weight can carry (both steps grow
    with e, so the largest e per w is all that matters).  It also covers subsequences no voxel can have -- a removal hit
    where the matching integration was missed -- which only raises it."""
    best = {0: 0.0}
    for s in signs:
        nxt = dict(best)  # (missed)
        for w, e in best.items():
            if s > 0:
                w2, e2 = w + 1, 0.0 if w == 0 else (w * e + 2 * w + 1) / (w + 1) + 1
            elif w == 0:
                continue
            else:
                w2, e2 = w - 1, 0.0 if w == 1 else (w * e + 2 * w + 1) / (w - 1) + 1
            nxt[w2] = max(nxt.get(w2, 0.0), e2)
        best = nxt
    return max(best.values()) * (1 + 2.0 ** -16)


def worst_error_bound(ops):
    """error_bound over every voxel there can be, in units of EPS.  ops: (sign, key) in order, key naming the op's frame
    and pose: a voxel is hit by every op of some keys and by no op of the others (rules 1 - 7 read nothing of the
    volume).  For short lists: 2^keys subsets."""
    keys = sorted({k for _, k in ops})
    worst = 0.0
    for mask in range(1 << len(keys)):
        hit = {k for i, k in enumerate(keys) if (mask >> i) & 1}
        e = error_bound([s for s, k in ops if k in hit])
        if e is not None:
            worst = max(worst, e)
    return worst
