"""THE SDF TRACKING RULE of include/icpk.h (K29) restated in numpy over a tsdf_model.Volume.  numpy is used only
elementwise, in float32, one rounding per operation in the order the header writes them, so that the device and
icpk_sdf_pixels are held against it bit for bit; the terms of an accepted pixel and the loop are float64.  The vertex,
the move and the cross normal are projective_model's, the cell and the trilinear value are tsdf_raycast_model's, the
canonical tree is gicp_model.canonical, and the loop's update is projective_model.update."""
import numpy as np

import gicp_model
import projective_model as jm
import tsdf_raycast_model as rm

F = np.float32
NO_DEPTH, OUTSIDE, UNKNOWN, TOO_FAR, NO_GRADIENT, NO_NORMAL, NORMAL = -1, -2, -3, -4, -5, -6, -7
CODES = (NO_DEPTH, OUTSIDE, UNKNOWN, TOO_FAR, NO_GRADIENT, NO_NORMAL, NORMAL)
OK, W_TOO_FEW_PAIRS, W_DEGENERATE = jm.OK, jm.W_TOO_FEW_PAIRS, jm.W_DEGENERATE
lerp = rm.lerp


def gradient(e, w):
    """rule 6: e[z][y][x] the eight corners, w = [w_x, w_y, w_z]; the gradient of rm.trilerp's interpolant, per voxel"""
    c00, c10 = lerp(e[0][0][0], e[0][0][1], w[0]), lerp(e[0][1][0], e[0][1][1], w[0])
    c01, c11 = lerp(e[1][0][0], e[1][0][1], w[0]), lerp(e[1][1][0], e[1][1][1], w[0])
    b0, b1 = lerp(c00, c10, w[1]), lerp(c01, c11, w[1])
    dx00, dx10 = e[0][0][1] - e[0][0][0], e[0][1][1] - e[0][1][0]
    dx01, dx11 = e[1][0][1] - e[1][0][0], e[1][1][1] - e[1][1][0]
    gx = lerp(lerp(dx00, dx10, w[1]), lerp(dx01, dx11, w[1]), w[2])
    gy = lerp(c10 - c00, c11 - c01, w[2])
    gz = b1 - b0
    return [gx, gy, gz]


def pixels(level, fx_s, cx_s, vol, pose, origin=None, max_abs_tsdf=1.0, min_weight=1, min_normal_cos=-2.0, normals=False):
    """Rules 1 - 8 for every pixel of the (rows, cols) uint16 image `level` seen through (fx_s, cx_s) -- the LEVEL's own
    intrinsics -- over the tsdf_model.Volume `vol` (origin: the one to use, default the volume's own).  Returns dict(cell
    (n,) int32: the cell or the code; value (n,) float32; terms (n, 28) float64, zero rows for a rejected pixel); with
    normals=True also normal (3, n) float32 and point (3, n) float32 (meaningful where cell >= 0)."""
    img = np.asarray(level, np.uint16)
    rows, cols = img.shape
    fx_s, cx_s, cap, min_cos = F(fx_s), F(cx_s), F(max_abs_tsdf), F(min_normal_cos)
    P = np.asarray(pose, np.float64).reshape(4, 4)
    R, t = P[:3, :3].astype(F), P[:3, 3].astype(F)
    n = rows * cols
    code = np.zeros(n, np.int32)  # 0: still in the running
    d = img.reshape(-1)
    rr = (np.arange(n) // cols).astype(F)
    cc = (np.arange(n) % cols).astype(F)

    class View:  # the volume as tsdf_raycast_model.cell reads it, at the origin to use
        dims, voxel = vol.dims, vol.voxel
    View.origin = vol.origin if origin is None else np.asarray(origin, F)
    with np.errstate(all="ignore"):
        code[d == 0] = NO_DEPTH
        vz = d.astype(F) / F(5000)
        vx = (cc - cx_s) * vz / fx_s
        vy = (rr - cx_s) * vz / fx_s
        p = jm.move(R, t, [vx, vy, vz])
        inr, i, w = rm.cell(View, p)
        code[(code == 0) & ~inr] = OUTSIDE
        dx, dy, dz = vol.dims
        at = i[0] + dx * (i[1] + dy * i[2])  # (0 where out of range: the gathers below stay in bounds)
        known = np.ones(n, bool)
        for plane in np.array(rm.corners(vol.weight >= min_weight, i)).reshape(8, -1):
            known &= plane
        code[(code == 0) & ~known] = UNKNOWN
        e = rm.corners(vol.tsdf, i)
        f = rm.trilerp(e, w)
        D = (f * vol.trunc).astype(F)
        code[(code == 0) & ~(np.abs(f) < cap)] = TOO_FAR
        g = gradient(e, w)
        length = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
        code[(code == 0) & ~(length > 0)] = NO_GRADIENT
        nv = [(x / length).astype(F) for x in g]
        if min_cos > F(-1):
            has, sn = jm.cross_normals(img, fx_s, cx_s)
            code[(code == 0) & ~has.reshape(-1)] = NO_NORMAL
            sn = [x.reshape(-1) for x in sn]
            flip = (sn[0] * vx + sn[1] * vy) + sn[2] * vz > 0
            sn = [np.where(flip, -x, x) for x in sn]
            w3 = [(R[k, 0] * sn[0] + R[k, 1] * sn[1]) + R[k, 2] * sn[2] for k in range(3)]
            cosv = (w3[0] * nv[0] + w3[1] * nv[1]) + w3[2] * nv[2]
            code[(code == 0) & ~(cosv >= min_cos)] = NORMAL
        ok = code == 0
        pd, nd = ([x.astype(np.float64) for x in y] for y in (p, nv))
        J = [pd[1] * nd[2] - pd[2] * nd[1], pd[2] * nd[0] - pd[0] * nd[2], pd[0] * nd[1] - pd[1] * nd[0], nd[0], nd[1], nd[2]]
        res = D.astype(np.float64)
        terms = np.zeros((n, 28))
        k = 0
        for x in range(6):
            for y in range(x, 6):
                terms[:, k] = J[x] * J[y]
                k += 1
        for x in range(6):
            terms[:, 21 + x] = J[x] * res
        terms[:, 27] = np.abs(D).astype(np.float64)
        terms[~ok] = 0.0
        terms = terms + 0.0  # (a term is ADDED to +0.0: a product that is -0.0 reads +0.0)
    out = dict(cell=np.where(ok, at, code).astype(np.int32), value=np.where(ok, D, F(0)).astype(F), terms=terms)
    if normals:
        out["normal"], out["point"] = np.array(nv, F), np.array(p, F)
    return out


def reduce(terms, cell):
    """(28 sums through the canonical tree, the accepted pixels)"""
    return gicp_model.canonical(terms), int((cell >= 0).sum())


def align(level, fx_s, cx_s, vol, pose, max_iterations=10, min_pairs=6, **kw):
    """The loop.  Returns dict(pose (4, 4), status, iterations, trace: list of dict(pose, sums, count, status))."""
    E = np.array(pose, np.float64).reshape(4, 4)
    E[3] = (0, 0, 0, 1)
    trace, status, done = [], OK, 0
    for _ in range(max_iterations):
        px = pixels(level, fx_s, cx_s, vol, E, **kw)
        sums, count = reduce(px["terms"], px["cell"])
        status, En = jm.update(sums, count, E, min_pairs)
        trace.append(dict(pose=E[:3].copy(), sums=sums, count=count, status=status))
        if status != OK:
            break
        E, done = En, done + 1
    return dict(pose=E, status=status, iterations=done, trace=trace)
