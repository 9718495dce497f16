"""TEST INFRASTRUCTURE: the three rules of K26 (include/icpk.h) restated in numpy, operation by operation -- THE INTENSITY
PYRAMID RULE over tests/pyramid_model.py's taps, THE VIEW GRADIENT RULE (K17's sums of tests/color_model.py over the
3 x 3 window of a ray-cast view; color_model.gradients_from_sums serves unchanged on them), and THE COLOURED PROJECTIVE
RULE (tests/projective_model.py decides the pair, K17's joint terms follow).  It never reads the library.  numpy
evaluates `a * b + c * d` as two rounded products and one rounded sum, never fused, which is what the header asks for."""
import numpy as np

import color_model as cm
import gicp_model
import projective_model as jm
import pyramid_model as pm

F = np.float32
FIX = 32768.0


# ---- THE INTENSITY PYRAMID RULE ---------------------------------------------------------------------------------------
def intensity_level_up(depth, inten, K):
    """Level l + 1 of the intensity from level l of both images."""
    img = np.asarray(depth, np.uint16)
    I = np.asarray(inten, F)
    rows, cols = img.shape
    r1, c1 = (rows + 1) // 2, (cols + 1) // 2
    d = np.zeros((rows + 2, cols + 2), np.int64)
    d[1:1 + rows, 1:1 + cols] = img
    q = np.zeros((rows + 2, cols + 2), np.int64)
    q[1:1 + rows, 1:1 + cols] = np.rint(I.astype(np.float64) * FIX).astype(np.int64)
    dc = d[1:1 + rows:2, 1:1 + cols:2]
    S, N = np.zeros((r1, c1), np.int64), np.zeros((r1, c1), np.int64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            sl = (slice(1 + dy, 1 + dy + 2 * r1 - 1, 2), slice(1 + dx, 1 + dx + 2 * c1 - 1, 2))
            dq = d[sl]
            ok = (dq != 0) & (np.abs(dq - dc) < K)
            w = (2 - abs(dy)) * (2 - abs(dx))
            S += np.where(ok, w, 0)
            N += np.where(ok, w * q[sl], 0)
    out = (N.astype(np.float64) / (np.maximum(S, 1).astype(np.float64) * FIX)).astype(F)
    return np.where(dc != 0, out, F(0)).astype(F)


def intensity_pyramid(depth, inten, levels, K=pm.DEFAULT_K):
    """The list of `levels` intensity images, level 0 first, beside pyramid_model.pyramid(depth, levels, K)."""
    ds = pm.pyramid(depth, levels, K)
    out = [np.array(inten, F)]
    for l in range(1, levels):
        out.append(intensity_level_up(ds[l - 1], out[-1], K))
    return out


# ---- THE VIEW GRADIENT RULE -------------------------------------------------------------------------------------------
def view_gradient_sums(view, radius):
    """(rows cols, 10) int64 of a view (8, rows, cols) float32: m, S_00 S_01 S_02 S_11 S_12 S_22, T_0 T_1 T_2"""
    v = np.asarray(view, F)
    rows, cols = v.shape[1:]
    pad = lambda a, fill: np.pad(a, 1, constant_values=fill)
    x, y, z, dep, inten = (pad(v[k], 0) for k in (0, 1, 2, 6, 7))
    hit = v[6] > 0
    n = v[3:6].astype(np.float64)
    usable = cm.usable_normals(v[3:6].reshape(3, -1)).reshape(rows, cols)
    r32, rd = F(radius), np.float64(F(radius))
    S = np.zeros((rows, cols, 10), np.int64)
    c = (slice(1, 1 + rows), slice(1, 1 + cols))
    with np.errstate(all="ignore"):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                s = (slice(1 + dy, 1 + dy + rows), slice(1 + dx, 1 + dx + cols))
                f = [a[s] - a[c] for a in (x, y, z)]
                dist = np.sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]).astype(F)
                nb = hit & (dep[s] > 0) & (dist <= r32)  # (the padding has depth 0: outside the view)
                S[..., 0] += nb
                use = nb & usable
                e = [a[s].astype(np.float64) - a[c].astype(np.float64) for a in (x, y, z)]
                h = (e[0] * n[0] + e[1] * n[1]) + e[2] * n[2]
                u = [e[a] - h * n[a] for a in range(3)]
                q = [np.where(use, np.rint((u[a] / rd) * FIX), 0).astype(np.int64) for a in range(3)]
                dc = np.where(use, np.rint((inten[s].astype(np.float64) - inten[c].astype(np.float64)) * FIX), 0).astype(np.int64)
                assert all((np.abs(t) <= 2 ** 15 + 128).all() for t in q) and (np.abs(dc) <= 2 ** 15).all()
                for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                    S[..., 1 + k] += q[a] * q[b]
                for a in range(3):
                    S[..., 7 + a] += q[a] * dc
    return S.reshape(-1, 10)


def view_gradients(view, radius, min_neighbors=4):
    """((3, rows, cols) float32 gradients, (rows cols, 10) int64 sums)"""
    v = np.asarray(view, F)
    S = view_gradient_sums(v, radius)
    g = cm.gradients_from_sums(S, v[3:6].reshape(3, -1), radius, min_neighbors)
    return g.reshape(3, *v.shape[1:]), S


# ---- THE COLOURED PROJECTIVE RULE -------------------------------------------------------------------------------------
def pixels(level, level_intensity, fx_s, cx_s, view, gradient, view_shape, fx_v, cx_v, view_pose, pose, max_dist=0.5,
           min_normal_cos=-2.0, lambda_geometric=cm.LAMBDA):
    """projective_model.pixels with the coloured rule 9.  view: (8, rows_v, cols_v); gradient: (3, rows_v, cols_v)."""
    out = jm.pixels(level, fx_s, cx_s, view, view_shape, fx_v, cx_v, view_pose, pose, max_dist, min_normal_cos)
    img = np.asarray(level, np.uint16)
    rows, cols = img.shape
    n = rows * cols
    pair = out["pixel"] >= 0
    j = np.where(pair, out["pixel"], 0).astype(np.int64)
    planes = [np.asarray(view[k], F).reshape(-1) for k in range(8)]
    grads = [np.asarray(gradient[k], F).reshape(-1) for k in range(3)]
    P = np.asarray(pose, np.float64).reshape(4, 4)
    R, t = P[:3, :3].astype(F), P[:3, 3].astype(F)
    fx_s, cx_s = F(fx_s), F(cx_s)
    rr = (np.arange(n) // cols).astype(F)
    cc = (np.arange(n) % cols).astype(F)
    lg = float(F(lambda_geometric))
    lc = 1.0 - lg
    with np.errstate(all="ignore"):
        vz = img.reshape(-1).astype(F) / F(5000)
        vx = (cc - cx_s) * vz / fx_s
        vy = (rr - cx_s) * vz / fx_s
        p = [a.astype(np.float64) for a in jm.move(R, t, [vx, vy, vz])]
        q = [planes[k][j].astype(np.float64) for k in range(3)]
        nv = [planes[3 + k][j].astype(np.float64) for k in range(3)]
        g = [grads[k][j].astype(np.float64) for k in range(3)]
        It = planes[7][j].astype(np.float64)
        Is = np.asarray(level_intensity, F).reshape(-1).astype(np.float64)
        e = [p[a] - q[a] for a in range(3)]
        h = (e[0] * nv[0] + e[1] * nv[1]) + e[2] * nv[2]
        G = [p[1] * nv[2] - p[2] * nv[1], p[2] * nv[0] - p[0] * nv[2], p[0] * nv[1] - p[1] * nv[0], nv[0], nv[1], nv[2]]
        u = [e[a] - h * nv[a] for a in range(3)]
        rc = (It + ((g[0] * u[0] + g[1] * u[1]) + g[2] * u[2])) - Is
        gn = (g[0] * nv[0] + g[1] * nv[1]) + g[2] * nv[2]
        M = [g[a] - gn * nv[a] for a in range(3)]
        Cc = [p[1] * M[2] - p[2] * M[1], p[2] * M[0] - p[0] * M[2], p[0] * M[1] - p[1] * M[0], M[0], M[1], M[2]]
        terms = np.zeros((n, 28))
        k = 0
        for a in range(6):
            for b in range(a, 6):
                terms[:, k] = lg * (G[a] * G[b]) + lc * (Cc[a] * Cc[b])
                k += 1
        for a in range(6):
            terms[:, 21 + a] = lg * (G[a] * h) + lc * (Cc[a] * rc)
        terms[:, 27] = out["dist"].astype(np.float64)
        terms[~pair] = 0.0
        terms = terms + 0.0  # (a term is ADDED to +0.0)
    out["terms"] = terms
    return out


def reduce(terms, pixel):
    return gicp_model.canonical(terms), int((pixel >= 0).sum())


def align(max_iterations=10, min_pairs=6, **args):
    """The loop: projective_model.align with the coloured evaluation.  args: pixels' keywords, `pose` the first estimate."""
    E = np.array(args.pop("pose"), np.float64).reshape(4, 4)
    E[3] = (0, 0, 0, 1)
    trace, status, done = [], jm.OK, 0
    for _ in range(max_iterations):
        px = pixels(pose=E, **args)
        sums, count = reduce(px["terms"], px["pixel"])
        status, En = jm.update(sums, count, E, min_pairs)
        trace.append(dict(pose=E[:3].copy(), sums=sums, count=count, status=status))
        if status != jm.OK:
            break
        E, done = En, done + 1
    return dict(pose=E, status=status, iterations=done, trace=trace)
