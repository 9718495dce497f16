"""TEST INFRASTRUCTURE: the Gauss-Newton systems of the seven linearised flavours (K5, K14, K17, K25, K26, K28, K29),
derived from the COST each flavour's section of include/icpk.h names and from nothing else.  It imports numpy only: none
of tests/*_model.py, not the library, not the oracle.  Everything is np.longdouble.

A flavour is a function residuals(x) -> (K, m): K already weighted residuals for each of m pairs or pixels, at the motion
x = (omega, t), p(x) = exp([omega]x) p + t with the exact exponential map -- the world-frame, left-multiplied motion the
loops compose as dT E.  The Jacobian is ALWAYS formed by central differences of that function (`jacobian`), never
analytically; H = J^T J and b = J^T r(0) follow, per pair (`linearise`).

The step H_MOTION = 2^-20: the truncation of a central difference of the exponential map is h^2 / 6 = 1.5e-13 relative
in J (h^2 / 3 = 3.0e-13 in H), and the rounding 2^-63 / h = 1.1e-13; both are below 1e-11.  The SDF flavour, whose cost
is only piecewise smooth, is probed with H_SDF = 1e-7 so that a probe stays inside its cell.

Beside the references the module holds the pieces every tolerance is computed from (the last section): the error of the
central difference itself, the float32 roundings a rule performs before it widens, propagated linearly, and the float64
arithmetic of the terms and of the canonical tree.  No number in it comes from a run of the code under test.

`wrong` selects a deliberately wrong reference (the tests demand that the code under test lies far from each):
"cross" the rotation turned the other way (every p x n reversed), "swap" lg and lc exchanged, "no_R" R_acc left off the
source normals, "negate" r negated, "right" dT composed on the right."""
import numpy as np

LD = np.longdouble
H_MOTION = LD(2) ** -20
H_SDF = LD(10) ** -7
U32, U64, ULD = LD(2) ** -24, LD(2) ** -53, LD(2) ** -64
N_LD_OPS = 32  # roundings of one residual evaluation (exponential map 9 + 6, motion 9, residual <= 8), each below ULD x scale


def ld(a):
    return np.asarray(a, LD)


# ---- the motion -------------------------------------------------------------------------------------------------------
def skew(w):
    w = ld(w)
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], LD)


def exp_so3(w):
    """exp([w]x) = I + (sin th / th) K + (2 sin^2(th / 2) / th^2) K^2: Rodrigues' formula without the cancelling 1 - cos"""
    w = ld(w)
    th = np.sqrt(w @ w)
    K = skew(w)
    if th == 0:
        return np.eye(3, dtype=LD)
    s = np.sin(th / 2)
    return np.eye(3, dtype=LD) + (np.sin(th) / th) * K + (2 * s * s / (th * th)) * (K @ K)


def move(x, p, wrong=None):
    """p(x) for (3, m) points"""
    x = ld(x)
    R = exp_so3(-x[:3] if wrong == "cross" else x[:3])
    return R @ ld(p) + x[3:, None]


# ---- central differences ----------------------------------------------------------------------------------------------
def jacobian(residuals, h=H_MOTION):
    """(r(0) (K, m), J (K, m, 6)) by central differences with step h"""
    h = LD(h)
    r0 = ld(residuals(np.zeros(6, LD)))
    J = np.zeros(r0.shape + (6,), LD)
    for k in range(6):
        x = np.zeros(6, LD)
        x[k] = h
        J[..., k] = (ld(residuals(x)) - ld(residuals(-x))) / (2 * h)
    return r0, J


def normal_equations(r0, J):
    """per pair: H (m, 6, 6) = sum_k J_k J_k^T and b (m, 6) = sum_k J_k r_k"""
    return np.einsum("kma,kmb->mab", J, J), np.einsum("kma,km->ma", J, r0)


def linearise(residuals, h=H_MOTION, wrong=None):
    """dict(r (K, m), J (K, m, 6), H (m, 6, 6), b (m, 6)) of a flavour, per pair"""
    r0, J = jacobian(residuals, h)
    H, b = normal_equations(r0, J)
    return dict(r=r0, J=J, H=H, b=-b if wrong == "negate" else b)


# ---- the costs --------------------------------------------------------------------------------------------------------
def p2l_residuals(p, q, n, wrong=None):
    """point-to-plane (K5, K25, K28): r = (p(x) - q) . n"""
    p, q, n = ld(p), ld(q), ld(n)
    return lambda x: ((move(x, p, wrong) - q) * n).sum(0)[None]


def patch(n, eps):
    """C(n) = I - (1 - eps) n n^T for (3, m) normals: (m, 3, 3)"""
    n = ld(n)
    return np.eye(3, dtype=LD)[None] - (1 - LD(eps)) * np.einsum("um,vm->muv", n, n)


def invert3(S):
    """(m, 3, 3) inverses: np.linalg.inv in float64, then two Newton steps M <- M (2 I - S M) in longdouble, which square
    its relative error (cond 2^-53 -> below 2^-64 for cond < 1e5)"""
    S = ld(S)
    M = ld(np.linalg.inv(S.astype(np.float64)))
    two = 2 * np.eye(3, dtype=LD)[None]
    for _ in range(2):
        M = np.einsum("muv,mvw->muw", M, two - np.einsum("muv,mvw->muw", S, M))
    return (M + M.transpose(0, 2, 1)) / 2


def chol3(M):
    """lower C with C C^T = M for (m, 3, 3) symmetric positive definite M"""
    C = np.zeros_like(M)
    for i in range(3):
        for j in range(i + 1):
            s = M[:, i, j] - (C[:, i, :j] * C[:, j, :j]).sum(1)
            C[:, i, j] = np.sqrt(s) if i == j else s / C[:, j, j]
    return C


def gicp_metric(a, b, R_acc, eps, form="cost", wrong=None):
    """M = S^-1 (m, 3, 3) and S.  form "cost": S = C(b) + R C(a) R^T, the paper's.  form "rule": that S less (R R^T - I),
    which is 2 I - (1 - eps) (m m^T + b b^T) with m = R a NOT renormalised: what include/icpk.h computes.  The two agree
    when R R^T = I."""
    R = np.eye(3, dtype=LD) if (R_acc is None or wrong == "no_R") else ld(R_acc).reshape(3, 3)
    a, b = ld(a), ld(b)
    S = patch(b, eps) + np.einsum("uv,mvw,xw->mux", R, patch(a, eps), R)
    if form != "cost":  # the deviation's own form: R I R^T taken for I
        S = S - (R @ R.T - np.eye(3, dtype=LD))[None]
    return invert3(S), S


def gicp_residuals(p, q, M, wrong=None):
    """plane-to-plane (K14): r = L (p(x) - q) with L^T L = M, M frozen: three residuals per pair"""
    p, q = ld(p), ld(q)
    L = chol3(M).transpose(0, 2, 1)  # L = C^T: L^T L = C C^T = M
    return lambda x: np.einsum("muv,vm->um", L, move(x, p, wrong) - q)


def colored_residuals(p, q, n, g, I_t, I_s, lambda_geometric, wrong=None):
    """colored (K17, K26): sqrt(lg) (p(x) - q) . n and sqrt(lc) (I_t + g . (pi(p(x)) - q) - I_s), pi the projection onto the
    tangent plane at q (pi(y) = y - ((y - q) . n) n); g frozen"""
    p, q, n, g, I_t, I_s = ld(p), ld(q), ld(n), ld(g), ld(I_t), ld(I_s)
    lg = LD(lambda_geometric)
    lc = 1 - lg
    if wrong == "swap":
        lg, lc = lc, lg

    def residuals(x):
        y = move(x, p, wrong)
        height = ((y - q) * n).sum(0)
        on_plane = y - height * n
        return np.stack([np.sqrt(lg) * height, np.sqrt(lc) * (I_t + (g * (on_plane - q)).sum(0) - I_s)])

    return residuals


class Trilinear:
    """The trilinear interpolant of a tsdf plane (dz, dy, dx), written afresh: cell centres at origin + (i + 0.5) voxel.
    A pixel's cell is FROZEN at what the code under test reports (`at` = x + dims_x (y + dims_y z), its lowest corner), and
    the cell's own polynomial is evaluated wherever the point lies."""

    def __init__(self, tsdf, origin, voxel, trunc):
        self.f = np.asarray(tsdf, np.float32)
        self.dims = self.f.shape[::-1]
        self.origin, self.voxel, self.trunc = ld(np.asarray(origin, np.float32)), LD(np.float32(voxel)), LD(np.float32(trunc))

    def index(self, at):
        at = np.asarray(at, np.int64)
        dx, dy, _ = self.dims
        return np.stack([at % dx, (at // dx) % dy, at // (dx * dy)])

    def corners(self, at):
        """e[x][y][z] (2, 2, 2, m) longdouble"""
        i = self.index(at)
        return ld(np.array([[[self.f[i[2] + z, i[1] + y, i[0] + x] for z in (0, 1)] for y in (0, 1)] for x in (0, 1)]))

    def fractions(self, p, at):
        return (ld(p) - self.origin[:, None]) / self.voxel - LD(0.5) - ld(self.index(at))

    def value(self, p, at, e=None):
        e = self.corners(at) if e is None else e
        w = self.fractions(p, at)
        cx = e[0] * (1 - w[0]) + e[1] * w[0]
        cy = cx[0] * (1 - w[1]) + cx[1] * w[1]
        return cy[0] * (1 - w[2]) + cy[1] * w[2]

    def cell_bounds(self, at):
        """What the tolerance of a pixel needs from its eight corners: A = max |e|; g1 (3, m): the largest |first
        difference| along each axis; m2 (3, 3, m): the largest |mixed second difference| of each pair of axes (0 on the
        diagonal: the interpolant is linear along an axis); t3 (m,): |the third mixed difference|"""
        e = self.corners(at)
        A = np.abs(e).reshape(8, -1).max(0)
        d = [e[1] - e[0], e[:, 1] - e[:, 0], e[:, :, 1] - e[:, :, 0]]  # (2, 2, m) each
        g1 = np.stack([np.abs(x).reshape(4, -1).max(0) for x in d])
        dxy, dxz, dyz = d[0][1] - d[0][0], d[0][:, 1] - d[0][:, 0], d[1][:, 1] - d[1][:, 0]  # (2, m) each
        m2 = np.zeros((3, 3, A.size), LD)
        m2[0, 1] = m2[1, 0] = np.abs(dxy).max(0)
        m2[0, 2] = m2[2, 0] = np.abs(dxz).max(0)
        m2[1, 2] = m2[2, 1] = np.abs(dyz).max(0)
        return A, g1, m2, np.abs(dxy[1] - dxy[0])


def sdf_residuals(field, p, at, wrong=None):
    """SDF (K29): r = trunc f(p(x))"""
    p = ld(p)
    e = field.corners(at)
    return lambda x: (field.trunc * field.value(move(x, p, wrong), at, e))[None]


def sdf_rows(field, p, at, h=H_SDF, wrong=None):
    """The numeric derivative of the SDF cost per pixel and the rule's system made from it: dict(D (m,) = r(0); J (m, 6):
    the central differences; kappa (m,) = |J[3:6]| = trunc |grad f| per metre; rows (m, 6) = J / kappa = [p x n ; n] with
    n the normalised numeric gradient; H (m, 6, 6) = rows rows^T; b (m, 6) = rows D)"""
    r0, J = jacobian(sdf_residuals(field, p, at, wrong), h)
    D, J = r0[0], J[0]
    kappa = np.sqrt((J[:, 3:] ** 2).sum(1))
    rows = J / kappa[:, None]
    H, b = np.einsum("ma,mb->mab", rows, rows), rows * D[:, None]
    return dict(D=D, J=J, kappa=kappa, rows=rows, H=H, b=-b if wrong == "negate" else b)


# ---- projective vertices ----------------------------------------------------------------------------------------------
def float_pose(E):
    """E's nine R and three t rounded to float once, widened"""
    E = np.asarray(E, np.float64).reshape(4, 4)
    return ld(E[:3, :3].astype(np.float32)), ld(E[:3, 3].astype(np.float32))


def vertices(level, fx_s, cx_s):
    """v = ((c - cx_s) z / fx_s, (r - cx_s) z / fx_s, z), z = d / 5000, for every pixel of the level: (3, rows cols),
    exact up to longdouble (cx_s for the rows as well: the rule's camera)"""
    img = np.asarray(level, np.uint16)
    rows, cols = img.shape
    fx, cx = LD(np.float32(fx_s)), LD(np.float32(cx_s))
    r, c = np.divmod(np.arange(rows * cols), cols)
    z = ld(img.reshape(-1)) / LD(5000)
    return np.stack([(ld(c) - cx) * z / fx, (ld(r) - cx) * z / fx, z])


def world_points(v, E):
    R, t = float_pose(E)
    return R @ v + t[:, None]


def world_point_error(v, E):
    """(3, m): the bound on |rule's float32 p - world_points|, counted from rules 2 and 3: v_z carries one rounding,
    v_x and v_y four (the difference, the product, v_z's own, the division); each product E_ab v_b one more; the three
    sums one each, of at most sum_b |E_ab v_b| + |t_a|."""
    R, t = float_pose(E)
    av = np.abs(v)
    k = ld([4, 4, 1])[:, None]
    s = np.abs(R) @ av
    return U32 * (np.abs(R) @ (k * av) + s + 3 * (s + np.abs(t)[:, None]))


# ---- the 6 x 6 --------------------------------------------------------------------------------------------------------
def unpack(sums):
    """the ICPK_NP2L layout: (H (6, 6) symmetric, b (6,), sum_dist)"""
    s = ld(sums)
    H = np.zeros((6, 6), LD)
    k = 0
    for a in range(6):
        for b in range(a, 6):
            H[a, b] = H[b, a] = s[k]
            k += 1
    return H, s[21:27].copy(), s[27]


def pack(H, b, sum_dist=0.0):
    """(28,) float64 in the ICPK_NP2L layout"""
    return np.array([H[a][b] for a in range(6) for b in range(a, 6)] + list(b) + [sum_dist], np.float64)


def triangle(H):
    """(..., 6, 6) -> (..., 21): the upper triangle row-major"""
    return np.stack([H[..., a, b] for a in range(6) for b in range(a, 6)], axis=-1)


def solve6(H, b):
    """H x = b by Gaussian elimination with partial pivoting in longdouble"""
    A = np.concatenate([ld(H).copy(), ld(b).reshape(6, 1)], axis=1)
    for c in range(6):
        piv = c + int(np.argmax(np.abs(A[c:, c])))
        A[[c, piv]] = A[[piv, c]]
        for r in range(c + 1, 6):
            A[r] -= (A[r, c] / A[c, c]) * A[c]
    x = np.zeros(6, LD)
    for r in range(5, -1, -1):
        x[r] = (A[r, 6] - A[r, r + 1:6] @ x[r + 1:]) / A[r, r]
    return x


def inverse6(H):
    return np.stack([solve6(H, np.eye(6, dtype=LD)[k]) for k in range(6)], axis=1)


def step(H, b):
    """the Gauss-Newton motion x = -H^-1 b"""
    return solve6(H, -ld(b))


def motion_matrix(x):
    T = np.eye(4, dtype=LD)
    T[:3, :3], T[:3, 3] = exp_so3(x[:3]), ld(x)[3:]
    return T


def stepped_pose(x, E0, wrong=None):
    """[exp([omega]x) | t] E_0 (wrong "right": E_0 [exp | t])"""
    T, E0 = motion_matrix(x), ld(E0).reshape(4, 4)
    return E0 @ T if wrong == "right" else T @ E0


# ---- what the tolerances are computed from ----------------------------------------------------------------------------
def cross_abs(a, b):
    """the sum of the absolute products of a x b along the last axis of two (..., 3) arrays of magnitudes"""
    return np.stack([a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], axis=-1)


def jacobian_scale(p, J):
    """SJ (K, m, 6): the magnitude each entry of J is evaluated at.  A residual linear in the point has the row
    [p x a ; a], a = J[3:6]; its rotational entries are differences of products below |p| |a|."""
    na = np.sqrt((J[..., 3:] ** 2).sum(-1))
    pn = np.sqrt((ld(p) ** 2).sum(0))
    return np.stack([na * pn] * 3 + [na] * 3, axis=-1)


def difference_error(SJ, r_scale, h=H_MOTION):
    """(K, m, 6): the error of the central difference itself: the truncation h^2 / 6 of the exponential map on a row of
    magnitude SJ, and N_LD_OPS roundings of ULD on a residual evaluated at magnitude r_scale (K, m), divided by h"""
    h = LD(h)
    return h * h / 6 * SJ + (N_LD_OPS * ULD / h) * ld(r_scale)[..., None]


def point_error(J, dp):
    """A point known only within dp (3, m) moves a residual linear in it, with row [p x a ; a]: (dr (K, m),
    dJ (K, m, 6)) = (|a| . dp, [dp x |a| ; 0])"""
    a = np.abs(J[..., 3:])
    dpt = ld(dp).T[None]
    return (a * dpt).sum(-1), np.concatenate([cross_abs(np.broadcast_to(dpt, a.shape), a), np.zeros_like(a)], axis=-1)


def product_error(r0, J, dJ, dr):
    """|J~ J~^T - J J^T| and |J~ r~ - J r| per pair for |J~ - J| <= dJ, |r~ - r| <= dr: (dH (m, 6, 6), db (m, 6))"""
    aJ, ar = np.abs(J), np.abs(r0)
    dH = np.einsum("kma,kmb->mab", aJ, dJ) + np.einsum("kma,kmb->mab", dJ, aJ) + np.einsum("kma,kmb->mab", dJ, dJ)
    db = np.einsum("kma,km->ma", dJ, ar + dr) + np.einsum("kma,km->ma", aJ, dr)
    return dH, db


def float64_error(SJ, r_scale, ops):
    """the float64 arithmetic of a pair's 27 terms: `ops` roundings of U64 on products of magnitude SJ_a SJ_b and
    SJ_a r_scale: (dH (m, 6, 6), db (m, 6))"""
    return (ops * U64 * np.einsum("kma,kmb->mab", SJ, SJ), ops * U64 * np.einsum("kma,km->ma", SJ, ld(r_scale)))


def tree_error(n, abs_terms):
    """the float64 canonical tree over n rows: n 2^-53 sum |term|, a bound for ANY order of summation"""
    return n * U64 * ld(abs_terms)


def sdf_float_error(field, p, at, dp, ref):
    """THE SDF TRACKING RULE's float32 roundings before it widens, for pixels at exact points p (3, m) known to the rule
    within dp; ref = sdf_rows(...).  Returns (d_rows (m, 6), dD (m,)).  Counted from rules 4 - 6 with the cell's own
    magnitudes: a = max |corner|, g_a the largest |first difference| along axis a, m_ab the largest |mixed second
    difference|.  lerp(u, v, w) = fl(u + fl(w fl(v - u))) passes its inputs' error on undiminished at most and adds three
    roundings: 2 |v - u| + max(|u|, |v|), in units of U32.
      fractions  w = fl(fl(fl(p - o) / voxel) - 0.5) - c: three roundings of at most G = |p - o| / voxel + 0.5, the last
                 subtraction exact: dw = dp / voxel + 3 U32 G
      c_yz       a lerp along x of corners: 2 g_x + a
      b_z        a lerp along y of two c: c's own, + 2 g_y + a: 2 g_x + 2 g_y + 2 a
      value      a lerp along z of two b, and D = fl(f trunc): dD = trunc (g . dw + U32 (2 g_x + 2 g_y + 2 g_z + 4 a))
      g_x        two levels of lerps over the four differences along x (one rounding of g_x each):
                 3 g_x + 2 m_xy + 2 m_xz
      g_y        a lerp along z of the differences of two c: 2 (2 g_x + a) + g_y, + 2 m_yz + g_y
      g_z        the difference of two b: 2 (2 g_x + 2 g_y + 2 a) + g_z
                 each plus what the fractions' error moves it by: sum_b m_ab dw_b
      normal     n = g / len, len five roundings and the division one: dn = |(I - n n^T) dg| / (len - |dg|) + 6 U32 |n|,
                 taken entry by entry with absolute values; len = |grad f| in cell units, from the reference: kappa voxel / trunc
      row        [p x n ; n] from the float p and n: dp x |n| + |p| x dn + dp x dn, and dn"""
    a, g1, m2, _ = field.cell_bounds(at)
    p = ld(p)
    G = np.abs(p - field.origin[:, None]) / field.voxel + LD(0.5)
    dw = ld(dp) / field.voxel + 3 * U32 * G
    gx, gy, gz = g1
    dD = field.trunc * ((g1 * dw).sum(0) + U32 * (2 * (gx + gy + gz) + 4 * a))
    own = U32 * np.stack([3 * gx + 2 * m2[0, 1] + 2 * m2[0, 2], 2 * a + 4 * gx + 2 * gy + 2 * m2[1, 2], 4 * a + 4 * gx + 4 * gy + gz])
    dg = np.einsum("abm,bm->am", m2, dw) + own
    length = ref["kappa"] * field.voxel / field.trunc
    room = length - np.sqrt((dg ** 2).sum(0))
    an = np.abs(ref["rows"][:, 3:]).T
    dn = np.where(room > 0, (dg + an * (an * dg).sum(0)) / np.where(room > 0, room, 1), LD(2)) + 6 * U32 * an
    ap, dpt, dnt = np.abs(p).T, ld(dp).T, dn.T
    return np.concatenate([cross_abs(dpt, an.T) + cross_abs(ap, dnt) + cross_abs(dpt, dnt), dnt], axis=1), dD


def sdf_difference_error(field, p, at, ref, h=H_SDF):
    """(m, 6): the error of ref["rows"] as the central difference made them.  Inside a cell r is a cubic in the point, so
    along a rotation the third derivative is below trunc (G1 P + 3 G2 P^2 + G3 P^3), P = |p|, G1, G2, G3 the sizes of the
    interpolant's first, second and third derivatives per metre; a translation along an axis is exact (f is linear in
    it).  The rounding is N_LD_OPS ULD trunc A / h.  rows = J / kappa with kappa = |J[3:6]| carries both, twice."""
    A, g1, m2, t3 = field.cell_bounds(at)
    h = LD(h)
    P = np.sqrt((ld(p) ** 2).sum(0))
    G1, G2, G3 = np.sqrt((g1 ** 2).sum(0)) / field.voxel, m2.sum((0, 1)) / field.voxel ** 2, t3 / field.voxel ** 3
    trunc3 = h * h / 6 * field.trunc * (G1 * P + 3 * G2 * P ** 2 + G3 * P ** 3)
    rnd = N_LD_OPS * ULD * field.trunc * (A + 1) / h
    dJ = np.concatenate([np.tile((trunc3 + rnd)[:, None], (1, 3)), np.tile(rnd[:, None], (1, 3))], axis=1)
    dk = np.sqrt((dJ[:, 3:] ** 2).sum(1))
    return (dJ + np.abs(ref["rows"]) * dk[:, None]) / (ref["kappa"] - dk)[:, None]


# ---- a flavour's reference and its tolerance, per pair ------------------------------------------------------------------
def norm3(a):
    return np.sqrt((ld(a) ** 2).sum(0))


def with_bounds(residuals, p, na, r_scale, r_eval, ops64, dp=None, wrong=None, h=H_MOTION):
    """linearise(residuals) plus dH (m, 6, 6), db (m, 6): the sum of the three parts of the tolerance.  na (K, m): the
    magnitude the direction of each residual is evaluated at (None: its own length); r_scale (K, m): the magnitude the
    rule evaluates the residual at; r_eval: the same for this module's own evaluation; ops64: the float64 roundings of a
    term; dp: the float32 error of the points (None: the points are exact floats)."""
    out = linearise(residuals, h, wrong)
    J = out["J"]
    na = np.sqrt((J[..., 3:] ** 2).sum(-1)) if na is None else ld(na)
    P = norm3(p)
    SJ = np.stack([na * P] * 3 + [na] * 3, axis=-1)
    dJ, dr = difference_error(SJ, r_eval, h), np.zeros_like(out["r"])
    if dp is not None:
        dr, dJ32 = point_error(J, dp)
        dJ = dJ + dJ32
    dH, db = product_error(out["r"], J, dJ, dr)
    eH, eb = float64_error(SJ, ld(r_scale) + dr, ops64)
    out.update(dH=dH + eH, db=db + eb)
    return out


def p2l_pairs(p, q, n, dp=None, wrong=None):
    """Point-to-plane.  float64 roundings of a term, from K5's text: a cross product entry 3, r 6 (three differences, three
    products and two sums, less the exact ones), a product of two of them 1 more: 12 covers J_a J_b (7) and J_a r (10)."""
    nn, e = norm3(n), norm3(ld(p) - ld(q))
    return with_bounds(p2l_residuals(p, q, n, wrong), p, None, (nn * e)[None], (nn * (norm3(p) + norm3(q)))[None], 12, dp, wrong)


def colored_pairs(p, q, n, g, I_t, I_s, lambda_geometric, dp=None, wrong=None):
    """Colored.  The photometric direction M = g - (g . n) n is formed by cancellation at magnitude |g| (1 + |n|^2), so
    that is the magnitude its row is held at.  float64 roundings of a term, from K17's text: M 7, a cross entry 3, C_a C_b
    1, the two weights 2, the sum 1, G_a G_b 7: 21; rc: u 5, its dot 5, two sums: 12, times C_a (10) and the weights: 26.
    32 covers both."""
    lg = LD(lambda_geometric)
    lc = 1 - lg
    nn, gn_, e = norm3(n), norm3(g), norm3(ld(p) - ld(q))
    na = np.stack([np.sqrt(lg) * nn, np.sqrt(lc) * gn_ * (1 + nn * nn)])
    photo = np.sqrt(lc) * (np.abs(ld(I_t)) + np.abs(ld(I_s)))
    r_scale = np.stack([na[0] * e, na[1] * e + photo])
    r_eval = np.stack([na[0] * (norm3(p) + norm3(q)), na[1] * (norm3(p) + norm3(q)) + photo])
    return with_bounds(colored_residuals(p, q, n, g, I_t, I_s, lambda_geometric, wrong), p, na, r_scale, r_eval, 32, dp, wrong)


def adjugate_inverse_error(S, M, a, b):
    """(m,): the bound on an entry of |rule's M - M|, M = S^-1 by the adjugate in float64 (K14's text), plus this module's
    own cond ULD.  With s = max |S|, mm = max(1, |a|^2, |b|^2): S_uv carries 12 roundings at mm and one at s; an entry of
    K two products of two S and a difference; det three products of S and K and two sums; M = K inv two more."""
    s = np.abs(S).max((1, 2))
    det = ld(np.linalg.det(S.astype(np.float64)))
    Mmax = np.abs(M).max((1, 2))
    Kmax = Mmax * det
    mm = np.maximum(1, np.maximum(norm3(a) ** 2, norm3(b) ** 2))
    dS = U64 * (12 * mm + s)
    dK = 4 * s * dS + 6 * U64 * s * s
    ddet = 3 * (s * dK + Kmax * dS) + 15 * U64 * s * Kmax
    return dK / det + Kmax * ddet / det ** 2 + 2 * U64 * Kmax / det + 16 * ULD * s * Mmax * Mmax


def gicp_pairs(p, q, a, b, R_acc, eps, form="cost", wrong=None):
    """Plane-to-plane.  M's own error (adjugate_inverse_error) enters J^T M J and J^T M r through J = [-[p]x | I], whose
    column sums are below 3 |p| and 3: 9 dM per entry.  float64 roundings of a term, from K14's text: B two products and a
    difference, A the same again, w five: 12."""
    M, S = gicp_metric(a, b, R_acc, eps, form, wrong)
    L = chol3(M)
    na = np.sqrt((L ** 2).sum(1)).T  # the rows of L^T = the columns of C
    e = norm3(ld(p) - ld(q))
    out = with_bounds(gicp_residuals(p, q, M, wrong), p, na, na * e, na * (norm3(p) + norm3(q)), 12, None, wrong)
    dM = adjugate_inverse_error(S, M, ld(R_acc).reshape(3, 3) @ ld(a) if R_acc is not None else a, b)
    P = norm3(p)
    Sp = np.stack([P] * 3 + [np.ones_like(P)] * 3, axis=-1)
    out["dH"] = out["dH"] + 9 * dM[:, None, None] * np.einsum("ma,mb->mab", Sp, Sp)
    out["db"] = out["db"] + 9 * (dM * e)[:, None] * Sp
    out.update(M=M, S=S)
    return out


def sdf_pixels(field, p, at, dp, wrong=None, h=H_SDF):
    """SDF: sdf_rows plus d_rows (m, 6), dD (m,), dH, db -- the float32 roundings of rules 4 - 6, the central difference's
    own error and 12 float64 roundings per term, as for point-to-plane -- and inside (m,) bool: every +-h probe of the
    pixel stays in its frozen cell (the margin is the motion of the point, h (|p| + 1), in cell units)."""
    ref = sdf_rows(field, p, at, h, wrong)
    d_rows, dD = sdf_float_error(field, p, at, dp, ref)
    d_rows = d_rows + sdf_difference_error(field, p, at, ref, h)
    rows, D = ref["rows"][None], ref["D"][None]
    dH, db = product_error(D, rows, d_rows[None], dD[None])
    P = norm3(p)
    SJ = np.stack([P] * 3 + [np.ones_like(P)] * 3, axis=-1)[None]
    eH, eb = float64_error(SJ, np.abs(D) + dD[None], 12)
    w = field.fractions(p, at)
    margin = LD(h) * (P + 1) / field.voxel
    ref.update(d_rows=d_rows, dD=dD, dH=dH + eH, db=db + eb, inside=((w > margin) & (w < 1 - margin)).all(0))
    return ref


def worst(got, want, bound):
    """the largest |got - want| / bound over all entries (entries whose bound and error are both 0 count as 0)"""
    err, bound = np.abs(ld(got) - ld(want)), ld(bound)
    with np.errstate(all="ignore"):
        ratio = np.where(err == 0, LD(0), err / bound)
    return float(ratio.max()) if ratio.size else 0.0


# ---- the image flavours: from the frozen association of the code under test to a reference ------------------------------
def projective_pixels(level, fx_s, cx_s, E, pixel, view, color=None, wrong=None):
    """K25 / K26 / K28.  pixel: per source pixel the view pixel it was paired with, or a negative code (the association is
    FROZEN at that); view: the planes x, y, z, nx, ny, nz, depth(, intensity) the code read; color: None, or dict(
    level_intensity, gradient (3, rows_v, cols_v), lambda_geometric).  Returns the bundle of p2l_pairs / colored_pairs
    over the accepted pixels in index order, plus index (their source pixels), dist and d_dist: the pairs' distances
    |p - m| and the bound on the rule's float32 one (the points' own error, and five roundings of rule 7)."""
    pixel = np.asarray(pixel).reshape(-1)
    i = np.nonzero(pixel >= 0)[0]
    j = pixel[i]
    planes = [np.asarray(a, np.float32).reshape(-1) for a in view]
    v = vertices(level, fx_s, cx_s)[:, i]
    p, dp = world_points(v, E), world_point_error(v, E)
    q, n = np.stack([planes[k][j] for k in range(3)]), np.stack([planes[k][j] for k in range(3, 6)])
    if color is None:
        out = p2l_pairs(p, q, n, dp, wrong)
    else:
        g = np.stack([np.asarray(a, np.float32).reshape(-1)[j] for a in color["gradient"]])
        I_s = np.asarray(color["level_intensity"], np.float32).reshape(-1)[i]
        out = colored_pairs(p, q, n, g, planes[7][j], I_s, np.float32(color["lambda_geometric"]), dp, wrong)
    dist = norm3(p - ld(q))
    out.update(index=i, dist=dist, d_dist=np.sqrt(3) * norm3(dp) + 5 * U32 * (dist + norm3(dp)))
    return out


def sdf_image(level, fx_s, cx_s, E, cell, field, wrong=None, h=H_SDF):
    """K29.  cell: per source pixel its cell or a negative code (FROZEN).  Returns sdf_pixels over the accepted pixels in
    index order, plus index."""
    cell = np.asarray(cell).reshape(-1)
    i = np.nonzero(cell >= 0)[0]
    v = vertices(level, fx_s, cx_s)[:, i]
    out = sdf_pixels(field, world_points(v, E), cell[i], world_point_error(v, E), wrong, h)
    out.update(index=i)
    return out
