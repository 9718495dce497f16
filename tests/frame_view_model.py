"""THE FRAME VIEW RULE of include/icpk.h (K28) restated in numpy.  numpy is used only elementwise, in float32, one
rounding per operation in the order the header writes them -- the vertex, the cross normal and the flip are
projective_model's own --, so that the device and icpk_frame_view_pixels are held against it bit for bit."""
import numpy as np

import projective_model as jm

F = np.float32


def view(level, fx_l, cx_l, pose, intensity=None):
    """Every pixel of the (rows, cols) uint16 image `level` seen through (fx_l, cx_l) -- the LEVEL's own intrinsics -- at
    the camera-to-world pose.  Returns dict(planes (8, rows, cols) float32: x, y, z, nx, ny, nz, depth, intensity;
    n_valid; n_no_normal; listed (rows, cols) bool)."""
    img = np.asarray(level, np.uint16)
    rows, cols = img.shape
    fx_l, cx_l = F(fx_l), F(cx_l)
    P = np.asarray(pose, np.float64).reshape(4, 4)
    R, t = P[:3, :3].astype(F), P[:3, 3].astype(F)
    rr = np.arange(rows).astype(F)[:, None] + np.zeros((1, cols), F)
    cc = np.arange(cols).astype(F)[None, :] + np.zeros((rows, 1), F)
    with np.errstate(all="ignore"):
        vz = img.astype(F) / F(5000)
        vx = (cc - cx_l) * vz / fx_l
        vy = (rr - cx_l) * vz / fx_l
        has, s = jm.cross_normals(img, fx_l, cx_l)
        flip = (s[0] * vx + s[1] * vy) + s[2] * vz > 0
        s = [np.where(flip, -x, x) for x in s]
        p = jm.move(R, t, [vx, vy, vz])
        n = [(R[a, 0] * s[0] + R[a, 1] * s[1]) + R[a, 2] * s[2] for a in range(3)]
    inten = np.zeros((rows, cols), F) if intensity is None else np.asarray(intensity, F).reshape(rows, cols)
    listed = (img != 0) & has
    planes = np.stack([np.where(listed, a, F(0)).astype(F) for a in (*p, *n, vz, inten)])
    # (a zeroed plane holds +0.0, never the -0.0 a product can give)
    return dict(planes=planes, n_valid=int(listed.sum()), n_no_normal=int(((img != 0) & ~has).sum()), listed=listed)
