"""TEST INFRASTRUCTURE: THE PLANE RULE of icpk_segment_planes (include/icpk.h, K34) restated in numpy -- the draws in
Python integers, the hypothesis planes and the counts in float64 numpy with every operation in the written association,
the nine sums through gicp_model.canonical (the canonical tree), the Jacobi eigen-solve operation for operation in scalar
float64.  The GPU tests compare the library against it bit for bit.  Never imported by the package.

brute_force() states the same rule a second time as a literal triple loop (rounds x hypotheses x points) in scalar
arithmetic, for clouds of a few hundred points; test_plane_host.py holds the two and icpk_segment_planes_host to one
another.
"""
import math

import numpy as np

import gicp_model as gm

M64 = 2 ** 64 - 1
DRAWS = 16
SWEEPS = 32
LINE_RATIO = 2.0 ** -20
FIELDS = ("labels", "out_index", "model", "info", "sums", "points")
NO_SAMPLE_SEED = 863  # sample(863, 0, 3) is None: the 16 draws of g = 0 at m = 3 take two values only
SPHERE_C, SPHERE_R = (5.35, 5.45, 7.3), 0.55  # config 2's sphere in the world frame (synth.render_room_depth + CAMERA_START)


def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, g, d, m):
    return (mix((seed + (g + 1) * 0x9E3779B97F4A7C15 + d * 0xD1B54A32D192ED03) & M64) >> 32) % m


def sample(seed, g, m):
    """the first three distinct positions among the 16 draws, or None"""
    c = []
    for d in range(DRAWS):
        v = draw(seed, g, d, m)
        if v not in c:
            c.append(v)
            if len(c) == 3:
                return c
    return None


def hypothesis(a, b, c, t):
    """(a float64 (3,), N (3,), G, valid) from three float32 points"""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    u, v = b - a, c - a
    N = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])
    L2 = (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]
    t = np.float64(np.float32(t))
    G = (t * t) * L2
    return a, N, G, bool(L2 > 0.0 and np.isfinite(G))


def hyp_inliers(P, a, N, G):
    """P (3, k) float64 -> (mask, e (3, k))"""
    e = P - a[:, None]
    s = (N[0] * e[0] + N[1] * e[1]) + N[2] * e[2]
    return s * s <= G, e


def orient(n):
    m = [abs(v) for v in n]
    k = 0
    if m[1] > m[k]:
        k = 1
    if m[2] > m[k]:
        k = 2
    return [-v for v in n] if n[k] < 0.0 else list(n)


def _div(a, b):
    """IEEE division of Python floats (x / 0 included)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(a):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(a)))


def eigen(C):
    """C = (c00, c01, c02, c11, c12, c22) -> (l0, l1, l2), the unit eigenvector of l0: the cyclic Jacobi of the rule"""
    A = [[C[0], C[1], C[2]], [C[1], C[3], C[4]], [C[2], C[4], C[5]]]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(SWEEPS):
        if A[0][1] == 0.0 and A[0][2] == 0.0 and A[1][2] == 0.0:
            break
        for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = A[p][q]
            if apq == 0.0:
                continue
            theta = _div(A[q][q] - A[p][p], 2.0 * apq)
            root = _sqrt(theta * theta + 1.0)
            t = _div(-1.0, root - theta) if theta < 0.0 else _div(1.0, root + theta)
            c = _div(1.0, _sqrt(t * t + 1.0))
            s = t * c
            tap = t * apq
            A[p][p] = A[p][p] - tap
            A[q][q] = A[q][q] + tap
            A[p][q] = A[q][p] = 0.0
            arp, arq = A[r][p], A[r][q]
            A[r][p] = A[p][r] = c * arp - s * arq
            A[r][q] = A[q][r] = s * arp + c * arq
            for k in range(3):
                vkp, vkq = V[k][p], V[k][q]
                V[k][p] = c * vkp - s * vkq
                V[k][q] = s * vkp + c * vkq
    d = [A[0][0], A[1][1], A[2][2]]
    i0 = 0
    if d[1] < d[i0]:
        i0 = 1
    if d[2] < d[i0]:
        i0 = 2
    x, y = [d[k] for k in range(3) if k != i0]
    l1, l2 = (x, y) if y >= x else (y, x)
    v = [V[k][i0] for k in range(3)]
    length = _sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    return (d[i0], l1, l2), [_div(c, length) for c in v]


def fit(S, count, a, N):
    """the refit: sums (9,), their count, the sample a (float32 (3,)), the hypothesis' normal -> (model (8,), fitted)"""
    S = [float(v) for v in S]
    a = [float(np.float32(v)) for v in a]
    N = [float(v) for v in N]
    k = float(count)
    with np.errstate(all="ignore"):
        mu = [_div(S[0], k), _div(S[1], k), _div(S[2], k)]
        C = [S[3] - _div(S[0] * S[0], k), S[4] - _div(S[0] * S[1], k), S[5] - _div(S[0] * S[2], k),
             S[6] - _div(S[1] * S[1], k), S[7] - _div(S[1] * S[2], k), S[8] - _div(S[2] * S[2], k)]
        l, n = eigen(C)
        n = orient(n)
        centre = [a[j] + mu[j] for j in range(3)]
        curvature = _div(l[0], (l[0] + l[1]) + l[2])
        fitted = count > 0 and not l[1] <= LINE_RATIO * l[2] and all(math.isfinite(v) for v in n + centre + list(l) + [curvature])
        if not fitted:
            length = _sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2])
            n = orient([_div(N[j], length) for j in range(3)])
            centre = a
            curvature = 0.0
        d = -((n[0] * centre[0] + n[1] * centre[1]) + n[2] * centre[2])
    return np.array(n + [d] + centre + [curvature], np.float64), fitted


def final_inliers(P, model, t):
    """P (3, k) float64 -> mask"""
    n, c = model[0:3], model[4:7]
    s = (n[0] * (P[0] - c[0]) + n[1] * (P[1] - c[1])) + n[2] * (P[2] - c[2])
    return np.abs(s) <= np.float64(np.float32(t))


def _finish(pts, labels, planes, unassigned, keep_inliers, select_plane, normals):
    n = pts.shape[1]
    fin = np.isfinite(pts).all(0)
    if keep_inliers:
        keep = (labels >= 0) & ((labels == select_plane) if select_plane >= 0 else True)
    else:
        keep = (labels < 0) & fin
    out = dict(labels=labels.astype(np.int32), out_index=np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32),
               model=np.array([p[0] for p in planes], np.float64).reshape(-1, 8),
               info=np.array([p[1] for p in planes], np.int32).reshape(-1, 6),
               sums=np.array([p[2] for p in planes], np.float64).reshape(-1, 9), n_planes=len(planes), n_unassigned=int(unassigned),
               n_out=int(keep.sum()), n_in=n, n_dropped=int((~fin).sum()), keep=keep, points=pts[:, keep])
    if normals is not None:
        out["normals"] = np.asarray(normals, np.float32).reshape(3, -1)[:, keep]
    return out


def segment(pts, distance_threshold=0.01, n_hypotheses=256, max_planes=4, min_inliers=1000, seed=0, keep_inliers=False,
            select_plane=-1, normals=None, counts_out=None):
    """dict(labels, out_index, model, info, sums, n_planes, n_unassigned, n_out, n_dropped, keep, points[, normals]) of the
    rule.  counts_out: a list that takes every round's c_h as an array (-1 for an invalid hypothesis)."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(3, -1)
    n = pts.shape[1]
    t, H = np.float32(distance_threshold), int(n_hypotheses)
    assert t > 0 and np.isfinite(t) and 1 <= H <= 65536 and 1 <= max_planes <= 16 and min_inliers >= 3
    fin = np.isfinite(pts).all(0)
    P64 = pts.astype(np.float64)
    labels = np.full(n, -1, np.int64)
    planes, unassigned = [], 0
    with np.errstate(all="ignore"):
        for r in range(max_planes):
            E = np.flatnonzero(fin & (labels < 0))
            m = E.size
            unassigned = m
            if m < 3 or m < min_inliers:
                break
            PE = P64[:, E]
            win = None  # (count, h, a, N, G, samples)
            counts = np.full(H, -1, np.int64)
            if counts_out is not None:
                counts_out.append(counts)
            for h in range(H):
                c = sample(seed, r * H + h, m)
                if c is None:
                    continue
                idx = [int(E[k]) for k in c]
                a, N, G, valid = hypothesis(pts[:, idx[0]], pts[:, idx[1]], pts[:, idx[2]], t)
                if not valid:
                    continue
                count = counts[h] = int(hyp_inliers(PE, a, N, G)[0].sum())
                if win is None or count > win[0]:
                    win = (count, h, a, N, G, idx)
            if win is None or win[0] < 3:
                break
            count, h, a, N, G, idx = win
            mask = np.zeros(n, bool)
            inl, e = hyp_inliers(PE, a, N, G)
            mask[E[inl]] = True
            e = e[:, inl]
            terms = np.zeros((n, 9))
            terms[mask] = np.stack([e[0], e[1], e[2], e[0] * e[0], e[0] * e[1], e[0] * e[2], e[1] * e[1], e[1] * e[2],
                                    e[2] * e[2]], axis=1)
            S = gm.canonical(terms)
            model, _ = fit(S, count, pts[:, idx[0]], N)
            fmask = final_inliers(PE, model, t)
            final = int(fmask.sum())
            if final < min_inliers:
                break
            labels[E[fmask]] = r
            planes.append((model, [h] + idx + [count, final], S))
            unassigned = m - final
    return _finish(pts, labels, planes, unassigned, keep_inliers, select_plane, normals)


def brute_force(pts, distance_threshold=0.01, n_hypotheses=256, max_planes=4, min_inliers=1000, seed=0, keep_inliers=False,
                select_plane=-1):
    """The rule once more as a literal triple loop in scalar float64 (small clouds only)."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(3, -1)
    n = pts.shape[1]
    t = float(np.float32(distance_threshold))
    X = [[float(pts[k, i]) for k in range(3)] for i in range(n)]  # (a float32 widens exactly)
    fin = [all(math.isfinite(v) for v in X[i]) for i in range(n)]
    labels = [-1] * n
    planes, unassigned = [], 0
    H = int(n_hypotheses)

    def in_hyp(p, a, N, G):
        e = [p[0] - a[0], p[1] - a[1], p[2] - a[2]]
        s = (N[0] * e[0] + N[1] * e[1]) + N[2] * e[2]
        return s * s <= G, e

    for r in range(max_planes):
        E = [i for i in range(n) if fin[i] and labels[i] < 0]
        m = len(E)
        unassigned = m
        if m < 3 or m < min_inliers:
            break
        win = None
        for h in range(H):
            c = sample(seed, r * H + h, m)
            if c is None:
                continue
            a, b, cc = X[E[c[0]]], X[E[c[1]]], X[E[c[2]]]
            u = [b[k] - a[k] for k in range(3)]
            v = [cc[k] - a[k] for k in range(3)]
            N = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
            L2 = (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]
            G = (t * t) * L2
            if not (L2 > 0.0 and math.isfinite(G)):
                continue
            count = 0
            for i in E:
                count += in_hyp(X[i], a, N, G)[0]
            if win is None or count > win[0]:
                win = (count, h, a, N, G, [E[k] for k in c])
        if win is None or win[0] < 3:
            break
        count, h, a, N, G, idx = win
        terms = np.zeros((n, 9))
        for i in E:
            ok, e = in_hyp(X[i], a, N, G)
            if ok:
                terms[i] = [e[0], e[1], e[2], e[0] * e[0], e[0] * e[1], e[0] * e[2], e[1] * e[1], e[1] * e[2], e[2] * e[2]]
        S = gm.canonical(terms)
        model, _ = fit(S, count, pts[:, idx[0]], N)
        nrm, c = [float(v) for v in model[0:3]], [float(v) for v in model[4:7]]
        fmask = [abs((nrm[0] * (X[i][0] - c[0]) + nrm[1] * (X[i][1] - c[1])) + nrm[2] * (X[i][2] - c[2])) <= t for i in E]
        final = sum(fmask)
        if final < min_inliers:
            break
        for i, f in zip(E, fmask):
            if f:
                labels[i] = r
        planes.append((model, [h] + idx + [count, final], S))
        unassigned = m - final
    return _finish(pts, np.array(labels, np.int64).reshape(n), planes, unassigned, keep_inliers, select_plane, None)


def same(a, b):
    """None if two records agree bit for bit, else the name of the first field that differs"""
    for key in FIELDS:
        u, v = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        if u.shape != v.shape or u.dtype != v.dtype:
            return f"{key} (shape / type: {u.shape} {u.dtype}, {v.shape} {v.dtype})"
        if u.tobytes() != v.tobytes():
            return key
    for key in ("n_planes", "n_out") + (("n_unassigned",) if "n_unassigned" in a and "n_unassigned" in b else ()):
        if a[key] != b[key]:
            return key
    return None


# ---- what the rule finds in config 2's target: the check both the host and the device tests make -----------------
WALLS = ((np.array([0.0, 0.0, 1.0]), -8.6), (np.array([1.0, 0.0, 0.0]), -2.9))  # z = 8.6 and x = 2.9 in the world frame
# Measured here with the model over seeds 0, 1, 2 (t 0.01, H 256, min_inliers 5000, max_planes 4): the worst angle to the
# analytic normal is 2.78e-5 rad (z = 8.6) and 1.75e-4 rad (x = 2.9), the worst offset error 1.50e-4 m and 1.52e-3 m.
# Asserted: three times the angle, twice the offset -- a margin against a change of synth only, since device = model.
ANGLE_TOL = (3 * 2.78e-5, 3 * 1.75e-4)
OFFSET_TOL = (2 * 1.50e-4, 2 * 1.52e-3)


def sphere_distance(p):
    return np.abs(np.linalg.norm(p.astype(np.float64) - np.array(SPHERE_C)[:, None], axis=0) - SPHERE_R)


def check_usefulness(r, tgt, seed):
    """exactly the two walls, each where the scene puts it; what remains is the sphere, and all of it"""
    assert r["n_planes"] == 2, seed
    for k, (nrm, d) in enumerate(WALLS):
        got = r["model"][k]
        angle = float(np.arctan2(np.linalg.norm(np.cross(nrm, got[:3])), float(nrm @ got[:3])))
        print(f"seed {seed} plane {k}: {r['info'][k, 5]} points, angle to the analytic normal {angle:.3e} rad, offset error "
              f"{abs(got[3] - d):.3e} m")
        assert angle <= ANGLE_TOL[k] and abs(got[3] - d) <= OFFSET_TOL[k]
    near_sphere = sphere_distance(tgt) <= 0.02
    assert sphere_distance(r["points"]).max() <= 0.02  # every remaining point is a sphere point
    assert int((near_sphere & (r["labels"] >= 0)).sum()) == 0  # and no sphere point was taken
    assert r["n_unassigned"] == r["n_out"] == int(near_sphere.sum())



# ---- the clouds of the tests --------------------------------------------------------------------------------------
def lattice(nx, ny, step=0.125, z=0.0, origin=(0.0, 0.0)):
    """an nx x ny lattice in the plane z: every coordinate a small multiple of a power of two, so every product of the
    rule is exact"""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")).reshape(2, -1).astype(np.float64) * step
    return np.stack([g[0] + origin[0], g[1] + origin[1], np.full(g.shape[1], z)]).astype(np.float32)


def noisy_plane(n, strays, seed=0, sigma=0.002, offset=(0.0, 0.0, 0.0)):
    """n points in all: a tilted plane with normal noise sigma plus `strays` uniform points, shuffled"""
    rng = np.random.default_rng(seed)
    k = n - strays
    uv = rng.uniform(-1.0, 1.0, (2, k))
    nrm = np.array([0.3, -0.2, 0.933])
    nrm /= np.linalg.norm(nrm)
    e1 = np.cross(nrm, [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    p = e1[:, None] * uv[0] + e2[:, None] * uv[1] + nrm[:, None] * rng.normal(0.0, sigma, k)
    p = np.concatenate([p, rng.uniform(-1.0, 1.0, (3, strays))], axis=1) + np.asarray(offset, np.float64)[:, None]
    return np.ascontiguousarray(p[:, rng.permutation(n)].astype(np.float32))


def edge_cases():
    """(name, points, keyword arguments) of the small clouds both the host and the device tests run: each is small enough
    for the host's O(P H n) program and for brute_force()."""
    rng = np.random.default_rng(23)
    t = 0.25
    flat = lattice(12, 10)
    tri = np.float32([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.5, 0.5, 0.5]])
    line = np.stack([np.arange(40) * 0.25, np.arange(40) * 0.5, np.arange(40) * -0.125]).astype(np.float32)
    edge = np.concatenate([flat, np.float32([[5.0, 5.125, 5.25], [0.0, 0.0, 0.0], [t, np.nextafter(np.float32(t), np.float32(1)), -t]])], axis=1)
    par = np.concatenate([lattice(8, 8, z=0.0), lattice(8, 8, z=2.0)], axis=1)
    par = par[:, np.argsort(np.tile(np.arange(64), 2), kind="stable")]  # the two planes interleaved
    cross = np.concatenate([lattice(14, 12), lattice(9, 9)[[2, 0, 1]] + np.float32([[0.5], [0.25], [0.125]])], axis=1)
    noisy = noisy_plane(400, 40, seed=5)
    nonfin = noisy.copy()
    nonfin[1, 17] = np.nan
    nonfin[0, 18] = np.inf
    nonfin[2, 399] = -np.inf
    nonfin[:, 0] = np.nan
    three = np.concatenate([noisy_plane(300, 10, seed=6), noisy_plane(200, 10, seed=7)[[1, 2, 0]] + np.float32([[3.0], [0.0], [0.0]]),
                            noisy_plane(150, 10, seed=8)[[2, 0, 1]] + np.float32([[0.0], [3.0], [0.0]])], axis=1)
    three = np.ascontiguousarray(three[:, rng.permutation(three.shape[1])])
    kw = dict(distance_threshold=0.01, n_hypotheses=32, max_planes=4, min_inliers=50, seed=1)
    lat = dict(distance_threshold=t, n_hypotheses=16, max_planes=4, min_inliers=20, seed=2)
    out = [("empty", np.zeros((3, 0), np.float32), kw), ("one", flat[:, :1], kw), ("two", flat[:, :2], kw),
           ("three, min_inliers 3", tri, dict(kw, min_inliers=3)), ("three, min_inliers 4", tri, dict(kw, min_inliers=4)),
           ("three, one hypothesis", tri, dict(kw, min_inliers=3, n_hypotheses=1, seed=9)),
           ("three, 16 draws without three distinct values", tri, dict(kw, min_inliers=3, n_hypotheses=1, seed=NO_SAMPLE_SEED)),
           ("three, the second hypothesis is the first valid one", tri, dict(kw, min_inliers=3, n_hypotheses=2, seed=NO_SAMPLE_SEED)),
           ("collinear", line, dict(kw, min_inliers=3)), ("identical", np.tile(np.float32([[1.0], [2.0], [3.0]]), (1, 64)), dict(kw, min_inliers=3)),
           ("non-finite", nonfin, kw), ("all non-finite", np.full((3, 7), np.nan, np.float32), dict(kw, min_inliers=3)),
           ("the <= edge", edge, lat), ("parallel lattices", par, dict(lat, distance_threshold=0.0625, n_hypotheses=64)), ("crossing lattices", cross, dict(lat, distance_threshold=0.0625)),
           ("scaled 1e-3", noisy * np.float32(1e-3), dict(kw, distance_threshold=1e-5)),
           ("scaled 1e3", noisy * np.float32(1e3), dict(kw, distance_threshold=10.0)),
           ("world offset", noisy_plane(400, 40, seed=5, offset=(5.0, 5.0, 5.0)), kw),
           ("one hypothesis", noisy, dict(kw, n_hypotheses=1, seed=3)),
           ("max_planes reached", three, dict(kw, max_planes=2)), ("three planes", three, kw),
           ("round discarded", three, dict(kw, min_inliers=150)),
           ("planes kept", three, dict(kw, keep_inliers=True)), ("plane 1 kept", three, dict(kw, keep_inliers=True, select_plane=1)),
           ("plane 3 kept: there is none", three, dict(kw, keep_inliers=True, select_plane=3))]
    return [(name, np.ascontiguousarray(p, np.float32), dict(k)) for name, p, k in out]
