"""CPU model of pose-graph optimisation (K18): include/icpk.h's rule restated in plain numpy, float64, OPERATION FOR
OPERATION: no libm but sqrt, every product and sum in the kernels' association (numpy only elementwise, where it can
neither fuse nor reassociate), the dot products through the canonical reduction tree -- so that the device can be held
against this model's bytes.  It restates the residual,
the line process, the analytic Jacobians, the node gather in ascending edge index, block-Jacobi PCG and Nielsen's
Levenberg-Marquardt with the pruning pass.  The device is held against this; this is held against central differences
and scipy (tests/test_posegraph_host.py).

An edge is a tuple (source, target, T (4, 4), info (6, 6), uncertain).  `reverse=True` walks every node's incident
edges in DESCENDING edge index: the same arithmetic in another summation order, which measures a graph's sensitivity
to rounding (s_graph)."""
import math

import numpy as np

PI_2 = 1.5707963267948966
RED_THREADS, RED_MAX_BLOCKS = 256, 256
_LANE = np.arange(64)


# ---- fixed-order arithmetic: what the kernels do, operation for operation -----------------------------------------
def _dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def _mat3(A, B):
    """A B for 3 x 3 blocks, every entry (a0 b0 + a1 b1) + a2 b2"""
    return (A[:, 0:1] * B[0:1, :] + A[:, 1:2] * B[1:2, :]) + A[:, 2:3] * B[2:3, :]


def _mv3(A, v):
    return (A[:, 0] * v[0] + A[:, 1] * v[1]) + A[:, 2] * v[2]


def _seq_mv(M, v):
    """M v with every row summed left to right from 0.0"""
    s = np.zeros(M.shape[0])
    for k in range(M.shape[1]):
        s = s + M[:, k] * v[k]
    return s


def _seq_dot(a, b):
    s = 0.0
    for k in range(len(a)):
        s = s + float(a[k]) * float(b[k])
    return s


def _block_sum(v):
    """the canonical tree over one workgroup: the wave64 butterfly (32, 16, ..., 1), then ((w0 + w1) + w2) + w3"""
    w = []
    for k in range(RED_THREADS // 64):
        x = np.array(v[64 * k:64 * k + 64], np.float64)
        for m in (32, 16, 8, 4, 2, 1):
            x = x + x[_LANE ^ m]
        w.append(float(x[0]))
    return ((w[0] + w[1]) + w[2]) + w[3]


def tree_sum(terms):
    """the canonical tree over len(terms) elements: element i goes to thread i mod (blocks x 256), a thread adds its
    elements in order from 0.0, every block sums its threads, and one block sums the blocks' slots"""
    n = len(terms)
    nb = min(max((n + RED_THREADS - 1) // RED_THREADS, 1), RED_MAX_BLOCKS)
    P = nb * RED_THREADS
    v = np.zeros(P)
    for i0 in range(0, n, P):
        chunk = np.asarray(terms[i0:i0 + P], np.float64)
        v[:len(chunk)] = v[:len(chunk)] + chunk
    slots = np.zeros(RED_THREADS)
    for b in range(nb):
        slots[b] = _block_sum(v[b * RED_THREADS:(b + 1) * RED_THREADS])
    return _block_sum(slots)


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def rod_coeffs(t2):
    """a = sin(th) / th, b = (1 - cos(th)) / th^2 from t2 = th^2: the power series in nested form, 20 terms, no libm"""
    pa = pb = 1.0
    for k in range(20, 0, -1):
        pa = 1.0 - (t2 / float((2 * k) * (2 * k + 1))) * pa
        pb = 1.0 - (t2 / float((2 * k + 1) * (2 * k + 2))) * pb
    return pa, 0.5 * pb


def atan_pos(x):
    """atan(x), x >= 0, from +, -, *, / and sqrt"""
    inv = x > 1.0
    if inv:
        x = 1.0 / x
    for _ in range(3):
        x = x / (1.0 + math.sqrt(1.0 + x * x))
    x2 = x * x
    p = 1.0 / 27.0
    for k in range(12, -1, -1):
        p = 1.0 / float(2 * k + 1) - x2 * p
    r = 8.0 * (x * p)
    return PI_2 - r if inv else r


def angle_pos(s, c):
    return atan_pos(s / c) if c > 0.0 else PI_2 + atan_pos(-c / s)


def rot_log(R):
    R = np.asarray(R, np.float64)
    v0, v1, v2 = float(R[2, 1] - R[1, 2]) / 2.0, float(R[0, 2] - R[2, 0]) / 2.0, float(R[1, 0] - R[0, 1]) / 2.0
    s = math.sqrt(_dot3(v0, v1, v2, v0, v1, v2))
    c = ((float(R[0, 0]) + float(R[1, 1])) + float(R[2, 2]) - 1.0) / 2.0
    if s < 1e-8 and c > 0.0:
        f = 1.0 + s * s / 6.0
    else:
        f = angle_pos(s, c) / s if s > 0.0 else 0.0
    return np.array([v0 * f, v1 * f, v2 * f])


def _xx(k, x, y, z, t2):
    """k [w]x^2 entries, as the kernels write them"""
    return k * (x * x - t2), k * (x * y), k * (x * z), k * (y * y - t2), k * (y * z), k * (z * z - t2)


def rot_exp(w):
    x, y, z = float(w[0]), float(w[1]), float(w[2])
    t2 = _dot3(x, y, z, x, y, z)
    a, b = rod_coeffs(t2)
    xx, xy, xz, yy, yz, zz = _xx(b, x, y, z, t2)
    return np.array([[1.0 + xx, -a * z + xy, a * y + xz], [a * z + xy, 1.0 + yy, -a * x + yz],
                     [-a * y + xz, a * x + yz, 1.0 + zz]])


def jl_inv(th):
    x, y, z = float(th[0]), float(th[1]), float(th[2])
    t2 = _dot3(x, y, z, x, y, z)
    t = math.sqrt(t2)
    if t < 1e-2:
        k = 1.0 / 12.0 + t2 / 720.0 + t2 * t2 / 30240.0
    else:
        a, b = rod_coeffs(t2)
        k = 1.0 / t2 - (1.0 + (1.0 - b * t2)) / (2.0 * t * (a * t))
    xx, xy, xz, yy, yz, zz = _xx(k, x, y, z, t2)
    return np.array([[1.0 + xx, 0.5 * z + xy, -0.5 * y + xz], [-0.5 * z + xy, 1.0 + yy, 0.5 * x + yz],
                     [0.5 * y + xz, -0.5 * x + yz, 1.0 + zz]])


def inv_pose(P):
    Q = np.eye(4)
    Q[:3, :3] = P[:3, :3].T
    Q[:3, 3] = -_mv3(Q[:3, :3], P[:3, 3])
    return Q


def exp_pose(d):
    D = np.eye(4)
    D[:3, :3] = rot_exp(d[:3])
    D[:3, 3] = d[3:]
    return D


def apply_step(d, P):
    """Exp(d) P as the trial kernel forms it"""
    R = rot_exp(d[:3])
    Q = np.array(P, np.float64)
    Q[:3, :3] = _mat3(R, P[:3, :3])
    Q[:3, 3] = _mv3(R, P[:3, 3]) + d[3:]
    return Q


def _edge_frames(Ps, Pt, T):
    Ti = inv_pose(T)
    RB = _mat3(Ps[:3, :3], Ti[:3, :3])
    tB = _mv3(Ps[:3, :3], Ti[:3, 3]) + Ps[:3, 3]
    RtT = np.ascontiguousarray(Pt[:3, :3].T)
    RE = _mat3(RtT, RB)
    tE = _mv3(RtT, tB - Pt[:3, 3])
    return RE, tE, tB, RtT


def residual(Ps, Pt, T):
    """r = (rotation vector of R_E, t_E), E = P_t^-1 P_s T^-1; also t_B of B = P_s T^-1."""
    RE, tE, tB, _ = _edge_frames(np.asarray(Ps, np.float64), np.asarray(Pt, np.float64), np.asarray(T, np.float64))
    return np.concatenate([rot_log(RE), tE]), tB


def jacobian_source(Pt, r, tB):
    """J_s = d r / d delta_s at delta = 0; J_t = -J_s."""
    RtT = np.ascontiguousarray(np.asarray(Pt, np.float64)[:3, :3].T)
    J = np.zeros((6, 6))
    J[:3, :3] = _mat3(jl_inv(r[:3]), RtT)
    J[3:, :3] = -_mat3(RtT, skew(tB))
    J[3:, 3:] = RtT
    return J


def line_weight(chi2, uncertain, mu):
    """(l, the edge's cost term)"""
    if uncertain and mu > 0.0:
        q = mu / (mu + chi2)
        return q * q, (q * q) * chi2 + mu * ((q - 1.0) * (q - 1.0))
    return 1.0, chi2


def edge_pass(poses, edges, mu, blocks=True):
    m = len(edges)
    chi2, l, term = np.zeros(m), np.zeros(m), np.zeros(m)
    A, b = np.zeros((m, 6, 6)), np.zeros((m, 6))
    for e, (s, t, T, info, unc) in enumerate(edges):
        info = np.asarray(info, np.float64)
        r, tB = residual(poses[s], poses[t], T)
        u = _seq_mv(info, r)
        chi2[e] = _seq_dot(r, u)
        l[e], term[e] = line_weight(float(chi2[e]), unc, mu)
        if blocks:
            J = jacobian_source(poses[t], r, tB)
            W = l[e] * info
            WJ = np.zeros((6, 6))  # column j: (l L) J[:, j], summed over m in order
            for k in range(6):
                WJ = WJ + W[:, k:k + 1] * J[k:k + 1, :]
            Ae = np.zeros((6, 6))  # A[i][j] = sum_k J[k][i] WJ[k][j]
            for k in range(6):
                Ae = Ae + J[k, :][:, None] * WJ[k, :][None, :]
            A[e] = Ae
            lu = l[e] * u
            be = np.zeros(6)
            for k in range(6):
                be = be + J[k, :] * lu[k]
            b[e] = be
    return chi2, l, tree_sum(term), A, b


def adjacency(n, edges, reverse=False):
    adj = [[] for _ in range(n)]
    for e, ed in enumerate(edges):
        adj[ed[0]].append((e, 1.0, ed[1]))
        adj[ed[1]].append((e, -1.0, ed[0]))
    return [a[::-1] for a in adj] if reverse else adj


def node_pass(n, adj, A, b):
    D, g = np.zeros((n, 6, 6)), np.zeros((n, 6))
    for i in range(n):
        for e, sign, _ in adj[i]:
            D[i] = D[i] + A[e]
            g[i] = g[i] + sign * b[e]
    return D, g


def evaluate(poses, edges, mu=0.0):
    """what icpk_pose_graph_evaluate returns: chi2, l, cost, gradient (n, 6)"""
    poses = np.asarray(poses, np.float64)
    chi2, l, cost, A, b = edge_pass(poses, edges, mu)
    _, g = node_pass(len(poses), adjacency(len(poses), edges), A, b)
    return chi2, l, cost, g


def _chol(D, lam):
    """the factor of D + lam diag D, read from D's lower triangle"""
    L = np.zeros((6, 6))
    for j in range(6):
        s = float(D[j, j]) + lam * float(D[j, j])
        for k in range(j):
            s = s - float(L[j, k]) * float(L[j, k])
        ok = s > 0.0
        d = math.sqrt(s) if ok else 1.0
        L[j, j] = d
        for i in range(j + 1, 6):
            t = float(D[i, j])
            for k in range(j):
                t = t - float(L[i, k]) * float(L[j, k])
            L[i, j] = t / d if ok else 0.0
    return L


def _chol_solve(L, r):
    y = [0.0] * 6
    for i in range(6):
        s = float(r[i])
        for k in range(i):
            s = s - float(L[i, k]) * y[k]
        y[i] = s / float(L[i, i])
    z = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - float(L[k, i]) * z[k]
        z[i] = s / float(L[i, i])
    return np.array(z)


def _node_dots(a, b):
    """per node the six products added in order from 0.0"""
    s = np.zeros(len(a))
    for k in range(6):
        s = s + a[:, k] * b[:, k]
    return s


def _chol_solve_all(L, r):
    """_chol_solve for every node at once (L (n, 6, 6), r (n, 6)): the same operations per node"""
    y = np.zeros_like(r)
    for i in range(6):
        s = r[:, i].copy()
        for k in range(i):
            s = s - L[:, i, k] * y[:, k]
        y[:, i] = s / L[:, i, i]
    z = np.zeros_like(r)
    for i in range(5, -1, -1):
        s = y[:, i].copy()
        for k in range(i + 1, 6):
            s = s - L[:, k, i] * z[:, k]
        z[:, i] = s / L[:, i, i]
    return z


def pcg(n, adj, A, D, g, lam, ref, tol, max_it):
    """(H + lam diag H) x = -g from x = 0, block-Jacobi preconditioned; returns x (n, 6) and the iterations"""
    diag = np.array([np.diag(D[i]) for i in range(n)])
    L = np.array([np.eye(6) if i == ref else _chol(D[i], lam) for i in range(n)])
    # a node's k-th incident edge, for all nodes that have one: the gather runs slot by slot, every node in its order
    slots = []
    for k in range(max(len(a) for a in adj)):
        idx = [i for i in range(n) if i != ref and len(adj[i]) > k]
        if idx:
            slots.append((np.array(idx), np.array([adj[i][k][0] for i in idx]), np.array([adj[i][k][2] for i in idx])))
    free = np.array([i != ref for i in range(n)])

    def hmul(p):
        q = np.zeros((n, 6))
        for idx, e, o in slots:
            d = p[idx] - p[o]
            s = np.zeros((len(idx), 6))
            for m in range(6):
                s = s + A[e][:, :, m] * d[:, m:m + 1]
            q[idx] = q[idx] + s
        q[free] = q[free] + (lam * diag[free]) * p[free]
        return q

    x = np.zeros((n, 6))
    r = -np.asarray(g, np.float64)
    if 0 <= ref < n:
        r[ref] = 0.0
    z = _chol_solve_all(L, r)
    p = z.copy()
    rz = tree_sum(_node_dots(r, z))
    g2 = tree_sum(_node_dots(r, r))
    if math.sqrt(g2) <= tol * math.sqrt(g2) or not rz > 0.0:
        return x, 0
    k = 0
    while k < max_it:
        q = hmul(p)
        pq = tree_sum(_node_dots(p, q))
        ok = pq > 0.0
        alpha = rz / pq if ok else 0.0
        x = x + alpha * p
        r = r - alpha * q
        z = _chol_solve_all(L, r)
        rzn = tree_sum(_node_dots(r, z))
        rr = tree_sum(_node_dots(r, r))
        p = z + (rzn / rz) * p
        rz = rzn
        k += 1
        if math.sqrt(rr) <= tol * math.sqrt(g2) or not ok or not rzn > 0.0:
            break
    return x, k


DEFAULTS = dict(max_iterations=100, max_pcg_iterations=200, pcg_tolerance=1e-8, tau=1e-3, cost_tolerance=1e-9,
                step_tolerance=1e-10, gradient_tolerance=1e-10, preference_loop_closure=0.0, edge_prune_threshold=0.25,
                reference_node=0, prune=False)


def _run_lm(poses, edges, p, reverse, trace, out):
    n, mu, ref = len(poses), p["preference_loop_closure"], p["reference_node"]
    adj = adjacency(n, edges, reverse)
    chi2, l, cost, A, b = edge_pass(poses, edges, mu)
    D, g = node_pass(n, adj, A, b)
    free = [i for i in range(n) if i != ref]
    if out["iterations"] == 0 and out["n_pruned"] == 0:
        out["initial_cost"] = cost
    lam, nu = p["tau"] * max([0.0] + [float(np.max(np.diag(D[i]))) for i in free]), 2.0
    out["final_lambda"] = lam
    converged = float(np.max(np.abs(g[free]))) < p["gradient_tolerance"]
    it = 0
    while it < p["max_iterations"] and not converged:
        x, k = pcg(n, adj, A, D, g, lam, ref, p["pcg_tolerance"], p["max_pcg_iterations"])
        x[ref] = 0.0
        pred = tree_sum([0.0 if i == ref else _seq_dot(x[i], (lam * np.diag(D[i])) * x[i] - g[i]) for i in range(n)])
        dmax = float(np.max(np.abs(x[free])))
        trial = np.array([poses[i] if i == ref else apply_step(x[i], poses[i]) for i in range(n)])
        chi2_t, l_t, cost_t, A_t, b_t = edge_pass(trial, edges, mu)
        D_t, g_t = node_pass(n, adj, A_t, b_t)
        rho = (cost - cost_t) / pred if pred > 0.0 else -1.0
        accepted = rho > 0.0
        out["iterations"] += 1
        out["pcg_iterations"] += k
        if accepted:
            rel = (cost - cost_t) / cost if cost > 0.0 else 0.0
            out["accepted"] += 1
            poses, cost, A, b, D, g, l = trial, cost_t, A_t, b_t, D_t, g_t, l_t
            c = 2.0 * rho - 1.0
            used, lam, nu = lam, lam * max(1.0 / 3.0, 1.0 - c * c * c), 2.0
            converged = rel < p["cost_tolerance"] or dmax < p["step_tolerance"] or \
                float(np.max(np.abs(g[free]))) < p["gradient_tolerance"]
        else:
            used, lam, nu = lam, lam * nu, 2.0 * nu
            converged = dmax < p["step_tolerance"]
        trace.append(dict(cost=cost, lam=used, pcg_iterations=k, accepted=accepted))
        out["final_lambda"] = lam
        it += 1
    return poses, cost, l, converged


def connected(n, edges, ref):
    """whether the edges join every node to `ref`"""
    adj = adjacency(n, edges)
    seen, todo = {ref}, [ref]
    while todo:
        for _, _, o in adj[todo.pop()]:
            if o not in seen:
                seen.add(o)
                todo.append(o)
    return len(seen) == n


def optimize(poses, edges, reverse=False, **params):
    """what icpk_pose_graph_optimize returns: dict(poses, weights, chi2, pruned, trace, converged, iterations, accepted,
    pcg_iterations, n_pruned, initial_cost, final_cost, final_lambda)"""
    p = dict(DEFAULTS)
    p.update(params)
    poses = np.array(poses, np.float64)
    edges = list(edges)
    out = dict(iterations=0, accepted=0, pcg_iterations=0, n_pruned=0, initial_cost=0.0, final_lambda=0.0)
    trace = []
    poses, cost, l, converged = _run_lm(poses, edges, p, reverse, trace, out)
    pruned = np.zeros(len(edges), bool)
    if p["prune"] and p["preference_loop_closure"] > 0.0:
        pruned = np.array([bool(ed[4]) and l[e] < p["edge_prune_threshold"] for e, ed in enumerate(edges)])
        kept = [ed for e, ed in enumerate(edges) if not pruned[e]]
        if pruned.any() and not connected(len(poses), kept, p["reference_node"]):
            pruned[:] = False  # (the rule: dropping them would cut a node off, so nothing is pruned)
        if pruned.any():
            out["n_pruned"] = int(pruned.sum())
            poses, cost, _, c2 = _run_lm(poses, kept, p, reverse, trace, out)
            converged = converged and c2
    chi2, l, _, _, _ = edge_pass(poses, edges, p["preference_loop_closure"], blocks=False)
    out.update(poses=poses, weights=l, chi2=chi2, pruned=pruned, trace=trace, converged=converged, final_cost=cost)
    return out
