"""THE PROJECTIVE RULE of include/icpk.h (K25) restated in numpy.  numpy is used only elementwise, in float32, one
rounding per operation in the order the header writes them, so that the device and icpk_projective_pixels are held
against it bit for bit; the terms of a pair and the loop are float64, the loop with numpy's sin / cos / sqrt.  The
canonical tree is gicp_model.canonical."""
import numpy as np

import gicp_model

F = np.float32
NO_DEPTH, BEHIND, OUTSIDE, NO_MODEL, TOO_FAR, NO_NORMAL, NORMAL = -1, -2, -3, -4, -5, -6, -7
CODES = (NO_DEPTH, BEHIND, OUTSIDE, NO_MODEL, TOO_FAR, NO_NORMAL, NORMAL)
OK, W_TOO_FEW_PAIRS, W_DEGENERATE = 0, 1, 2


def invert_pose(pose):
    """icpk_tsdf_invert_pose: (Q (3, 3), s (3,)) float32, inverted in double and rounded once"""
    P = np.asarray(pose, np.float64).reshape(4, 4)
    Q = P[:3, :3].T.astype(F)
    s = np.array([-((P[0, r] * P[0, 3] + P[1, r] * P[1, 3]) + P[2, r] * P[2, 3]) for r in range(3)]).astype(F)
    return Q, s


def move(R, t, v):
    """R v + t in the form of integration rule 2; v: three float32 arrays"""
    return [((R[a, 0] * v[0] + R[a, 1] * v[1]) + R[a, 2] * v[2]) + t[a] for a in range(3)]


def cross_normals(img, fx, cx):
    """K4's ICPK_NORMALS_CROSS normal of every pixel: (has (rows, cols) bool, [n_x, n_y, n_z] float32, 0 where not)"""
    rows, cols = img.shape
    has = np.zeros((rows, cols), bool)
    n = [np.zeros((rows, cols), F) for _ in range(3)]
    if rows < 3 or cols < 3:
        return has, n
    r = np.arange(1, rows - 1).astype(F)[:, None]
    c = np.arange(1, cols - 1).astype(F)[None, :]
    dE, dW, dS, dN = img[1:-1, 2:], img[1:-1, :-2], img[2:, 1:-1], img[:-2, 1:-1]
    ok = (dE != 0) & (dW != 0) & (dS != 0) & (dN != 0)
    with np.errstate(all="ignore"):
        zE, zW, zS, zN = (d.astype(F) / F(5000) for d in (dE, dW, dS, dN))
        one = F(1)
        xE, yE = ((c + one) - cx) * zE / fx, (r - cx) * zE / fx
        xW, yW = ((c - one) - cx) * zW / fx, (r - cx) * zW / fx
        xS, yS = (c - cx) * zS / fx, ((r + one) - cx) * zS / fx
        xN, yN = (c - cx) * zN / fx, ((r - one) - cx) * zN / fx
        ax, ay, az = xE - xW, yE - yW, zE - zW
        bx, by, bz = xS - xN, yS - yN, zS - zN
        vx, vy, vz = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx
        l = np.sqrt((vx * vx + vy * vy) + vz * vz)
        ok &= l > 0
        for k, v in enumerate((vx, vy, vz)):
            n[k][1:-1, 1:-1] = np.where(ok, v / l, F(0))
    has[1:-1, 1:-1] = ok
    return has, n


def pixels(level, fx_s, cx_s, view, view_shape, fx_v, cx_v, view_pose, pose, max_dist=0.5, min_normal_cos=-2.0):
    """Rules 1 - 9 for every pixel of the (rows, cols) uint16 image `level` seen through (fx_s, cx_s) -- the LEVEL's own
    intrinsics.  view: (7+, rows_v, cols_v) float32 planes x, y, z, nx, ny, nz, depth.  Returns dict(pixel (n,) int32: the
    view pixel or the code; dist (n,) float32; terms (n, 28) float64, zero rows without a pair)."""
    img = np.asarray(level, np.uint16)
    rows, cols = img.shape
    rows_v, cols_v = view_shape
    planes = [np.asarray(view[k], F).reshape(-1) for k in range(7)]
    fx_s, cx_s, fx_v, cx_v, max_dist, min_cos = F(fx_s), F(cx_s), F(fx_v), F(cx_v), F(max_dist), F(min_normal_cos)
    P = np.asarray(pose, np.float64).reshape(4, 4)
    R, t = P[:3, :3].astype(F), P[:3, 3].astype(F)
    Q, s = invert_pose(view_pose)
    n = rows * cols
    code = np.zeros(n, np.int32)      # 0: still in the running
    d = img.reshape(-1)
    rr = (np.arange(n) // cols).astype(F)
    cc = (np.arange(n) % cols).astype(F)
    with np.errstate(all="ignore"):
        code[d == 0] = NO_DEPTH
        vz = d.astype(F) / F(5000)
        vx = (cc - cx_s) * vz / fx_s
        vy = (rr - cx_s) * vz / fx_s
        p = move(R, t, [vx, vy, vz])
        q = move(Q, s, p)
        code[(code == 0) & ~(q[2] > 0)] = BEHIND
        u = (q[0] * fx_v) / q[2] + cx_v
        v = (q[1] * fx_v) / q[2] + cx_v
        a, b = u + F(0.5), v + F(0.5)
        inside = (a >= 0) & (a < F(cols_v)) & (b >= 0) & (b < F(rows_v))
        code[(code == 0) & ~inside] = OUTSIDE
        live = code == 0
        j = np.zeros(n, np.int64)
        j[live] = b[live].astype(np.int64) * cols_v + a[live].astype(np.int64)
        code[live & ~(planes[6][j] > 0)] = NO_MODEL
        m = [planes[k][j] for k in range(3)]
        e = [p[k] - m[k] for k in range(3)]
        dist = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]).astype(F)
        code[(code == 0) & ~(dist < max_dist)] = TOO_FAR
        nv = [planes[3 + k][j] for k in range(3)]
        if min_cos > F(-1):
            has, sn = cross_normals(img, fx_s, cx_s)
            code[(code == 0) & ~has.reshape(-1)] = NO_NORMAL
            sn = [x.reshape(-1) for x in sn]
            flip = (sn[0] * vx + sn[1] * vy) + sn[2] * vz > 0
            sn = [np.where(flip, -x, x) for x in sn]
            w = [(R[k, 0] * sn[0] + R[k, 1] * sn[1]) + R[k, 2] * sn[2] for k in range(3)]
            cosv = (w[0] * nv[0] + w[1] * nv[1]) + w[2] * nv[2]
            code[(code == 0) & ~(cosv >= min_cos)] = NORMAL
        pair = code == 0
        pd, md, nd = ([x.astype(np.float64) for x in y] for y in (p, m, nv))
        J = [pd[1] * nd[2] - pd[2] * nd[1], pd[2] * nd[0] - pd[0] * nd[2], pd[0] * nd[1] - pd[1] * nd[0], nd[0], nd[1], nd[2]]
        res = ((pd[0] - md[0]) * nd[0] + (pd[1] - md[1]) * nd[1]) + (pd[2] - md[2]) * nd[2]
        terms = np.zeros((n, 28))
        k = 0
        for x in range(6):
            for y in range(x, 6):
                terms[:, k] = J[x] * J[y]
                k += 1
        for x in range(6):
            terms[:, 21 + x] = J[x] * res
        terms[:, 27] = dist.astype(np.float64)
        terms[~pair] = 0.0
        terms = terms + 0.0  # (a term is ADDED to +0.0: a product that is -0.0 reads +0.0)
    return dict(pixel=np.where(pair, j, code).astype(np.int32), dist=np.where(pair, dist, F(0)).astype(F), terms=terms)


def reduce(terms, pixel):
    """(28 sums through the canonical tree, the pair count)"""
    return gicp_model.canonical(terms), int((pixel >= 0).sum())


def solve_p2l(sums):
    """csrc/solve_impl.h solve_p2l: (dR (3, 3), dt (3,)) or None when the normal equations are not positive definite"""
    A = np.zeros((6, 6))
    k = 0
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = sums[k]
            k += 1
    dmax = max(0.0, A.diagonal().max())
    L = np.zeros((6, 6))
    for i in range(6):
        for j in range(i + 1):
            s = A[i, j]
            for m in range(j):
                s -= L[i, m] * L[j, m]
            if i == j:
                if not s > 1e-12 * dmax:
                    return None
                L[i, i] = np.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    y, x = np.zeros(6), np.zeros(6)
    for i in range(6):
        s = -sums[21 + i]
        for m in range(i):
            s -= L[i, m] * y[m]
        y[i] = s / L[i, i]
    for i in range(5, -1, -1):
        s = y[i]
        for m in range(i + 1, 6):
            s -= L[m, i] * x[m]
        x[i] = s / L[i, i]
    a0, a1, a2 = x[:3]
    th2 = (a0 * a0 + a1 * a1) + a2 * a2
    th = np.sqrt(th2)
    if th < 1e-9:
        A1, B1 = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        A1, B1 = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    K = np.array([[0, -a2, a1], [a2, 0, -a0], [-a1, a0, 0]], np.float64)
    dR = np.zeros((3, 3))
    for r in range(3):
        for c in range(3):
            k2 = (K[r, 0] * K[0, c] + K[r, 1] * K[1, c]) + K[r, 2] * K[2, c]
            dR[r, c] = (1.0 if r == c else 0.0) + (A1 * K[r, c] + B1 * k2)
    return dR, x[3:].copy()


def compose(dR, dt, E):
    """E' = dT E in double with 3-term products; E: (3, 4) or (4, 4), the result has E's shape"""
    E = np.asarray(E, np.float64)
    out = E.copy()
    for r in range(3):
        for c in range(3):
            out[r, c] = (dR[r, 0] * E[0, c] + dR[r, 1] * E[1, c]) + dR[r, 2] * E[2, c]
        out[r, 3] = ((dR[r, 0] * E[0, 3] + dR[r, 1] * E[1, 3]) + dR[r, 2] * E[2, 3]) + dt[r]
    return out


def update(sums, count, E, min_pairs=6):
    """one iteration of the loop rule from the sums at E: (status, E')"""
    if count < min_pairs:
        return W_TOO_FEW_PAIRS, np.array(E, np.float64)
    sol = solve_p2l(sums)
    if sol is None:
        return W_DEGENERATE, np.array(E, np.float64)
    return OK, compose(sol[0], sol[1], E)


def align(level, fx_s, cx_s, view, view_shape, fx_v, cx_v, view_pose, pose, max_iterations=10, max_dist=0.5,
          min_normal_cos=-2.0, min_pairs=6):
    """The loop.  Returns dict(pose (4, 4), status, iterations, trace: list of dict(pose, sums, count, status))."""
    E = np.array(pose, np.float64).reshape(4, 4)
    E[3] = (0, 0, 0, 1)
    trace, status, done = [], OK, 0
    for _ in range(max_iterations):
        px = pixels(level, fx_s, cx_s, view, view_shape, fx_v, cx_v, view_pose, E, max_dist, min_normal_cos)
        sums, count = reduce(px["terms"], px["pixel"])
        status, En = update(sums, count, E, min_pairs)
        trace.append(dict(pose=E[:3].copy(), sums=sums, count=count, status=status))
        if status != OK:
            break
        E, done = En, done + 1
    return dict(pose=E, status=status, iterations=done, trace=trace)
