"""Float64 restatement of robust alignment (include/icpk.h, icpk_set_robust): the selection of the cut tau and the
median m, the weights, the weighted Kabsch and point-to-plane solves and the loop around them.

Test infrastructure only.  It reads the oracle's Python API (nn_bruteforce, transform_points, solve_p2l) and never
the library.  Sums are plain float64 numpy sums, not the canonical tree: the model pins the selection and the weights
exactly (tau, m, counts, weights) and the sums and transforms to rounding.
"""
import math

import numpy as np

NONE, HUBER, TUKEY = 0, 1, 2
FIXED, MEDIAN = 0, 1
IDENTITY = dict(kernel=NONE, scale=1.0, scale_mode=FIXED, trim=1.0)


def ranks(n, trim):
    """(k, ceil(n/2)): the 1-based ranks of tau and m among n accepted distances"""
    k = math.ceil(float(np.float64(np.float32(trim))) * n)
    return min(max(k, 1), n), (n + 1) // 2


def select(d_acc, trim):
    """tau and m (float32) of the accepted distances; 0 and 0 when there are none"""
    d_acc = np.asarray(d_acc, np.float32)
    n = d_acc.size
    if n == 0:
        return np.float32(0), np.float32(0)
    k, mr = ranks(n, trim)
    return np.partition(d_acc, k - 1)[k - 1], np.partition(d_acc, mr - 1)[mr - 1]


def scale_of(cfg, m):
    if cfg["scale_mode"] == MEDIAN:
        return float(np.float32(cfg["scale"])) * 1.4826 * float(m)
    return float(np.float32(cfg["scale"]))


def weights(d, tau, c, kernel):
    """w(d) in float64 for accepted distances d: 0 beyond the cut, else the kernel's weight"""
    x = np.asarray(d, np.float32).astype(np.float64)
    w = np.ones_like(x)
    if kernel == HUBER:
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(x <= c, 1.0, c / x)
    elif kernel == TUKEY:
        with np.errstate(divide="ignore", invalid="ignore"):
            r = x / c
            u = 1.0 - r * r
            w = np.where(x == 0.0, 1.0, np.where(x < c, u * u, 0.0))
    return np.where(np.asarray(d, np.float32) <= tau, w, 0.0)


def accepted_mask(dist, max_dist, idx=None, nrm=None):
    acc = np.asarray(dist, np.float32) < np.float32(max_dist)
    if nrm is not None:
        j = np.where(acc, idx, 0)
        acc &= ~((nrm[0, j] == 0) & (nrm[1, j] == 0) & (nrm[2, j] == 0))
    return acc


def robust_weights(dist, max_dist, cfg, idx=None, nrm=None):
    """one sweep: (accepted mask, w for every query (0 where not accepted), tau, m, c)"""
    acc = accepted_mask(dist, max_dist, idx, nrm)
    d_acc = np.asarray(dist, np.float32)[acc]
    tau, m = select(d_acc, cfg["trim"])
    c = scale_of(cfg, m)
    w = np.zeros(acc.size)
    w[acc] = weights(d_acc, tau, c, cfg["kernel"])
    return acc, w, tau, m, c


def sums_kabsch(src, tgt, idx, dist, acc, w):
    """ICPK_NSUM_W in plain float64 sums"""
    a = src[:, acc].astype(np.float64)
    b = tgt[:, idx[acc]].astype(np.float64)
    ww = w[acc]
    diff = (src[:, acc] - tgt[:, idx[acc]]).astype(np.float64)
    s = [np.sum(ww * b[r] * a[c]) for r in range(3) for c in range(3)]
    s += [np.sum(ww * diff[c]) for c in range(3)]
    s += [np.sum(np.asarray(dist, np.float32)[acc].astype(np.float64))]
    s += [np.sum(ww * a[c]) for c in range(3)] + [np.sum(ww * b[c]) for c in range(3)]
    s += [np.sum(ww), float(np.count_nonzero(ww > 0))]
    return np.array(s)


def sums_p2l(src, tgt, nrm, idx, dist, acc, w):
    """ICPK_NP2L_W in plain float64 sums"""
    p = src[:, acc].astype(np.float64)
    q = tgt[:, idx[acc]].astype(np.float64)
    n = nrm[:, idx[acc]].astype(np.float64)
    ww = w[acc]
    J = [p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2]]
    r = ((p[0] - q[0]) * n[0] + (p[1] - q[1]) * n[1]) + (p[2] - q[2]) * n[2]
    s = [np.sum(ww * J[a] * J[b]) for a in range(6) for b in range(a, 6)]
    s += [np.sum(ww * J[a] * r) for a in range(6)]
    s += [np.sum(np.asarray(dist, np.float32)[acc].astype(np.float64)), np.sum(ww), float(np.count_nonzero(ww > 0))]
    return np.array(s)


def solve_kabsch(sums):
    """weighted centred Kabsch from ICPK_NSUM_W (rigid_transform_3D.py:9-40 with weights): R, t mapping a onto b"""
    W = sums[19]
    ca, cb = sums[13:16] / W, sums[16:19] / W
    sab = np.array([[sums[3 * c + r] for c in range(3)] for r in range(3)])  # sum w a_r b_c
    H = sab - W * np.outer(ca, cb)
    U, _, Vt = np.linalg.svd(H)
    R = Vt.T @ U.T
    if np.linalg.det(R) < 0:
        Vt[2] *= -1
        R = Vt.T @ U.T
    return R, cb - R @ ca


class KdNN:
    """the NN of icp.cpp:566-593 (lowest float distance, lowest index on ties) through a k-d tree's candidates, each
    re-measured with the reference's float distance; the oracle's brute force when scipy is missing"""

    def __init__(self, tgt, oracle):
        self.tgt = tgt
        self.oracle = oracle
        try:
            from scipy.spatial import cKDTree

            self.tree = cKDTree(tgt.T.astype(np.float64))
        except ImportError:  # pragma: no cover
            self.tree = None

    def __call__(self, src):
        if self.tree is None:  # pragma: no cover
            return self.oracle.nn_bruteforce(src, self.tgt, threads=self.oracle.max_threads())
        _, cand = self.tree.query(src.T.astype(np.float64), k=8)
        t = self.tgt[:, cand]  # (3, n, 8)
        dx, dy, dz = (src[k][:, None] - t[k] for k in range(3))
        s = (dx.astype(np.float64) ** 2 + dy.astype(np.float64) ** 2) + dz.astype(np.float64) ** 2
        d = np.sqrt(s.astype(np.float32))
        m = d.min(axis=1, keepdims=True)  # lowest distance, then lowest index
        best = np.where(d == m, cand, np.iinfo(np.int64).max).min(axis=1)
        return best.astype(np.int32), m[:, 0]


def align(src, tgt, oracle, cfg, iterations=20, max_dist=0.75, nrm=None, min_pairs=3):
    """fixed-iteration robust loop (Kabsch, or point-to-plane with nrm): T (4x4 float64 from the float motions, as
    the library accumulates them), the kept count and tau of every iteration, and the status (1: fell back)"""
    nn = KdNN(tgt, oracle)
    cur = np.asarray(src, np.float32).copy()
    Tk = np.eye(4)
    kept, cuts = [], []
    for _ in range(iterations):
        idx, dist = nn(cur)
        acc, w, tau, m, c = robust_weights(dist, max_dist, cfg, idx, nrm)
        nk = int(np.count_nonzero(w > 0))
        if nk < min_pairs:
            return Tk, kept, cuts, 1
        kept.append(nk)
        cuts.append(tau)
        if nrm is None:
            R, t = solve_kabsch(sums_kabsch(cur, tgt, idx, dist, acc, w))
        else:
            R, t, rc = oracle.solve_p2l(sums_p2l(cur, tgt, nrm, idx, dist, acc, w)[:28])
            assert rc == 0
        Rf, tf = R.astype(np.float32), t.astype(np.float32)
        cur = oracle.transform_points(cur, Rf, tf)
        step = np.eye(4)
        step[:3, :3], step[:3, 3] = Rf, tf
        Tk = step @ Tk
    return Tk, kept, cuts, 0


def contaminated_pair(n=10000, seed=1, share=0.25):
    """synth.frustum_pair with `share` of the source points displaced by 0.2-0.5 m in a random direction: still
    inside the 0.75 m gate, so the plain loop lets them pull the solve"""
    from icp_slam_prototype_amd import synth

    p = synth.frustum_pair(n=n, seed=seed)
    rng = np.random.default_rng(seed + 100)
    src = p["source"].astype(np.float64)
    bad = rng.choice(n, int(share * n), replace=False)
    v = rng.normal(size=(3, bad.size))
    v /= np.linalg.norm(v, axis=0)
    src[:, bad] += v * rng.uniform(0.2, 0.5, bad.size)
    p["source"] = src.astype(np.float32)
    p["outliers"] = bad
    return p


def motion_error(T, p):
    """rotation (Frobenius norm of the difference) and translation (m) error of T, the estimated source -> target
    motion, against the pair's truth: source = R (target - c) + c + s, so target = R^T (source - c - s) + c"""
    R, s = p["R_true"], p["t_true"]
    c = p["target"].astype(np.float64).mean(axis=1)
    tinv = c - R.T @ (c + s)
    return float(np.linalg.norm(T[:3, :3] - R.T)), float(np.linalg.norm(T[:3, 3] - tinv))
