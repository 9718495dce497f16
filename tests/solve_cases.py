"""Seeded cases for csrc/solve_impl.h and the ctypes wrapper of its test probe (tests/cpp/solve_probe.hip), shared by
tests/test_solve_probe_host.py (host entry points, no GPU) and tests/test_gpu_solve_device.py (device vs host).

Every generator returns arrays of cases built to reach one branch of the solve: exact rank 0 / 1 / 2 moments, repeated
singular values, reflections, |det| on both sides of polar3's 1e-7 switch, the 1e-290 / 1e290 guards, subnormal and
non-finite entries, point sets whose centring cancels, and SPD systems on both sides of solve_p2l's pivot test and its
Taylor switch.  The high-precision references (mpmath, 50 digits) live here too."""
import ctypes as C

import mpmath
import numpy as np

from icp_slam_prototype_amd import build

DIGITS = 50

_i32p, _i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
_f32p, _f64p = C.POINTER(C.c_float), C.POINTER(C.c_double)


class Probe:
    """solve_impl.h over arrays of n cases: on_device=False runs the host code, True one thread per case on GPU 0."""

    def __init__(self):
        self.lib = C.CDLL(build.program("solve_probe"))
        for name in ("polar3", "svd3", "solve_reference", "solve_kabsch", "solve_p2l", "invert3f", "mul3f",
                     "sqrt_f64", "div_f64", "sqrt_f32", "div_f32"):
            getattr(self.lib, "probe_" + name).restype = C.c_int

    def _call(self, name, on_device, n, *arrays):
        ptrs = []
        for a in arrays:
            assert a.flags.c_contiguous and a.shape[0] == n, name
            ptr = {np.dtype(np.int32): _i32p, np.dtype(np.int64): _i64p, np.dtype(np.float32): _f32p,
                   np.dtype(np.float64): _f64p}[a.dtype]
            ptrs.append(a.ctypes.data_as(ptr))
        rc = getattr(self.lib, "probe_" + name)(int(bool(on_device)), int(n), *ptrs)
        assert rc == 0, f"probe_{name}: hip error {rc}"

    def polar3(self, A, on_device=False):
        A = np.ascontiguousarray(A, np.float64).reshape(-1, 9)
        n = len(A)
        ok, Q = np.zeros(n, np.int32), np.zeros((n, 9))
        self._call("polar3", on_device, n, A, ok, Q)
        return ok, Q.reshape(n, 3, 3)

    def svd3(self, A, on_device=False):
        A = np.ascontiguousarray(A, np.float64).reshape(-1, 9)
        n = len(A)
        U, S, V = np.zeros((n, 9)), np.zeros((n, 3)), np.zeros((n, 9))
        self._call("svd3", on_device, n, A, U, S, V)
        return U.reshape(n, 3, 3), S, V.reshape(n, 3, 3)

    def solve_reference(self, M, on_device=False):
        M = np.ascontiguousarray(M, np.float32).reshape(-1, 9)
        n = len(M)
        R = np.zeros((n, 9), np.float32)
        self._call("solve_reference", on_device, n, M, R)
        return R.reshape(n, 3, 3)

    def solve_kabsch(self, cnt, sa, sb, sab, on_device=False):
        cnt = np.ascontiguousarray(cnt, np.int64).reshape(-1)
        n = len(cnt)
        sa = np.ascontiguousarray(sa, np.float64).reshape(n, 3)
        sb = np.ascontiguousarray(sb, np.float64).reshape(n, 3)
        sab = np.ascontiguousarray(sab, np.float64).reshape(n, 9)
        R, t = np.zeros((n, 9)), np.zeros((n, 3))
        self._call("solve_kabsch", on_device, n, cnt, sa, sb, sab, R, t)
        return R.reshape(n, 3, 3), t

    def solve_p2l(self, sums, on_device=False):
        sums = np.ascontiguousarray(sums, np.float64).reshape(-1, 28)
        n = len(sums)
        ok, R, t = np.zeros(n, np.int32), np.zeros((n, 9)), np.zeros((n, 3))
        self._call("solve_p2l", on_device, n, sums, ok, R, t)
        return ok, R.reshape(n, 3, 3), t

    def invert3f(self, Rin, on_device=False):
        Rin = np.ascontiguousarray(Rin, np.float32).reshape(-1, 9)
        n = len(Rin)
        ok, out = np.zeros(n, np.int32), np.zeros((n, 9), np.float32)
        self._call("invert3f", on_device, n, Rin, ok, out)
        return ok, out.reshape(n, 3, 3)

    def mul3f(self, A, B, on_device=False):
        A = np.ascontiguousarray(A, np.float32).reshape(-1, 9)
        B = np.ascontiguousarray(B, np.float32).reshape(-1, 9)
        n = len(A)
        out = np.zeros((n, 9), np.float32)
        self._call("mul3f", on_device, n, A, B, out)
        return out.reshape(n, 3, 3)

    def sqrt(self, a, on_device=False):
        a = np.ascontiguousarray(a)
        out = np.zeros_like(a)
        self._call("sqrt_f64" if a.dtype == np.float64 else "sqrt_f32", on_device, len(a), a, out)
        return out

    def div(self, a, b, on_device=False):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b, a.dtype)
        out = np.zeros_like(a)
        self._call("div_f64" if a.dtype == np.float64 else "div_f32", on_device, len(a), a, b, out)
        return out


# ---------------------------------------------------------------------------------------------- generators --
def random_rotation(rng, n):
    """(n, 3, 3) proper rotations (QR of Gaussian matrices, sign-fixed)."""
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[np.linalg.det(q) < 0, :, 2] *= -1
    return q


PERMS = np.array([np.eye(3)[list(p)] for p in ((0, 1, 2), (1, 2, 0), (2, 0, 1), (1, 0, 2), (0, 2, 1), (2, 1, 0))])


def legacy_reference_moments():
    """The 3000 moments of tests/test_abi.py::test_polar_solve_matches_jacobi_oracle_on_random_moments (same seed,
    same draws), float32, with their kind (4: almost rank 1, 5: exactly rank 1 before rounding)."""
    rng = np.random.default_rng(123)
    out, kinds = [], []
    for t in range(3000):
        c = rng.normal(5, 1, 3)
        kind = t % 6
        noise = [0.3, 1e-2, 1e-4, 3.0, 1e-7, 0.0][kind]
        M = (np.outer(c, c) * (0 if kind == 3 else 1) + noise * rng.normal(0, 1, (3, 3))) * 10.0 ** rng.uniform(-3, 6)
        if t % 7 == 0:
            M = -M
        out.append(M.astype(np.float32))
        kinds.append(kind)
    return np.stack(out), np.array(kinds)


def det_switch_diagonals(dtype, kmax):
    """diag(1, 1, d) and its row / sign permutations, |d| = 1e-7 (1 +- 2^-k): the scaled determinant polar3 tests
    against 1e-7 is d exactly (largest entry 1, cofactor products exact), so each case lies on a known side."""
    out, side = [], []
    for k in range(1, kmax + 1):
        for sgn in (-1.0, 1.0):
            d = dtype(1e-7 * (1.0 + sgn * 2.0 ** -k))
            if float(d) == 1e-7:
                continue
            for p in range(len(PERMS)):
                for neg in (1.0, -1.0):
                    for scale in (1.0, 2.0 ** -20, 2.0 ** 30):  # powers of two: the scaled matrix is unchanged
                        M = (PERMS[p] @ np.diag([1.0, 1.0, float(d)]) * neg * scale).astype(dtype)
                        out.append(M)
                        side.append(float(d) >= 1e-7)
    return np.stack(out), np.array(side)


def structured_moments(rng, dtype=np.float32):
    """Exact-rank, repeated-singular-value, reflected, ill-conditioned, guard-edge, subnormal and non-finite moments.
    Returns (M (n, 3, 3), labels list)."""
    fin = np.finfo(dtype)
    cases, labels = [], []

    def add(M, label):
        cases.append(np.asarray(M, np.float64).astype(dtype))
        labels.append(label)

    add(np.zeros((3, 3)), "rank0")
    add(-np.zeros((3, 3)), "rank0")
    for i in range(60):
        u, v = rng.normal(size=3), rng.normal(size=3)
        if i % 3 == 0:  # exactly representable rank-1: small-integer outer products
            u, v = rng.integers(-4, 5, 3).astype(float), rng.integers(-4, 5, 3).astype(float)
            if not u.any() or not v.any():
                u, v = np.array([1.0, 2.0, 3.0]), np.array([1.0, -1.0, 2.0])
        add(np.outer(u, v) * 10.0 ** rng.uniform(-3, 5), "rank1")
        add(np.outer(u, u) * (i + 1), "rank1")
    for i in range(60):  # exactly rank 2: a zero row / column, or integer rows with row 2 = row 0 + row 1
        M = rng.integers(-6, 7, (3, 3)).astype(float)
        if i % 3 == 0:
            M[2] = 0.0
        elif i % 3 == 1:
            M[:, rng.integers(0, 3)] = 0.0
        else:
            M[2] = M[0] + M[1]
        add(M * 10.0 ** rng.integers(-3, 4), "rank2")
        add(-M, "rank2")
    for i in range(40):  # repeated singular values
        s = float(10.0 ** rng.uniform(-3, 5))
        add(np.eye(3) * s, "sigmaI")
        add(-np.eye(3) * s, "sigmaI")
        add(PERMS[i % 6] * s, "sigmaI")  # a permutation: orthogonal, det +-1
        eps = float(10.0 ** rng.uniform(-12, -1))
        add(np.diag([1.0, 1.0, eps]) * s, "diag11eps")
        Rr = random_rotation(rng, 1)[0]
        add(Rr @ np.diag([1.0, 1.0, eps]) @ random_rotation(rng, 1)[0].T * s, "diag11eps_rot")
        add(Rr * s, "sigmaI_rot")
    for i in range(120):  # conditioning up to past polar3's switch (cond ~1e7) and on to the SVD's 1e-15 cut
        lc = rng.uniform(0, 9)
        sv = np.array([1.0, 10.0 ** -rng.uniform(0, lc), 10.0 ** -lc])
        M = random_rotation(rng, 1)[0] @ np.diag(sv) @ random_rotation(rng, 1)[0].T * 10.0 ** rng.uniform(-2, 4)
        add(M, "cond")
        add(-M, "cond_reflect")
        Mr = M.copy()
        Mr[:, 2] *= -1
        add(Mr, "cond_reflect")
    # guards and special values
    for v in (fin.tiny, fin.tiny * 2 ** -10, fin.smallest_subnormal, fin.smallest_subnormal * 3):
        add(np.eye(3) * float(v), "subnormal")
        add(rng.normal(size=(3, 3)) * float(v) * 100, "subnormal")
        M = rng.normal(size=(3, 3))
        M[rng.integers(0, 3), rng.integers(0, 3)] = float(v)
        add(M, "subnormal_mixed")
    if dtype == np.float64:
        for g in (1e290, 1e-290):
            for v in (g, np.nextafter(g, 0.0), np.nextafter(g, np.inf)):
                M = rng.normal(size=(3, 3)) * 0.5
                M[0, 0] = 0.0
                M = M * v  # others stay below, amax = v exactly
                M[0, 0] = v
                add(M, "guard")
                add(np.eye(3) * v, "guard")
        add(np.eye(3) * 1e300, "huge")
        add(rng.normal(size=(3, 3)) * 1e300, "huge")
    else:
        add(np.eye(3) * float(fin.max), "huge")
        add(rng.normal(size=(3, 3)) * 1e37, "huge")
    for bad in (np.nan, np.inf, -np.inf):
        for pos in ((0, 0), (1, 2), (2, 2)):
            M = rng.normal(size=(3, 3))
            M[pos] = bad
            add(M, "nonfinite")
        add(np.full((3, 3), bad), "nonfinite")
    return np.stack(cases), labels


def reference_cases(seed=7):
    """Every float32 moment the reference flavour is tested on: (M (n, 3, 3) float32, labels)."""
    rng = np.random.default_rng(seed)
    Ms, labels = structured_moments(rng, np.float32)
    D, _ = det_switch_diagonals(np.float32, 23)
    L, kinds = legacy_reference_moments()
    M = np.concatenate([Ms, D.astype(np.float32), L])
    return M, labels + ["det_switch"] * len(D) + [f"legacy{k}" for k in kinds]


def polar_cases(seed=8):
    """float64 inputs of polar3 / svd3: (A (n, 3, 3), labels)."""
    rng = np.random.default_rng(seed)
    Ms, labels = structured_moments(rng, np.float64)
    D, _ = det_switch_diagonals(np.float64, 50)
    L, kinds = legacy_reference_moments()
    return np.concatenate([Ms, D, L.astype(np.float64)]), labels + ["det_switch"] * len(D) + [f"legacy{k}" for k in kinds]


def kabsch_point_sets(seed=9):
    """(name, A (3, n), B (3, n)) float64 point sets where Kabsch's centring cancels or its SVD is degenerate."""
    rng = np.random.default_rng(seed)
    sets = []
    for off in (np.array([5.0, 5.0, 5.0]), np.array([1e4, -1e4, 1e4])):
        for rep in range(4):
            Rt = random_rotation(rng, 1)[0]
            tt = rng.normal(0, 0.1, 3)
            n = int(rng.integers(8, 400))
            s = rng.uniform(-1, 1, n)
            d = rng.normal(size=3)
            A = np.outer(d, s) + off[:, None]                                   # exactly collinear
            sets.append(("collinear", A, Rt @ A + tt[:, None]))
            A = np.vstack([rng.uniform(-1, 1, (2, n)), np.zeros((1, n))])
            A = random_rotation(rng, 1)[0] @ A + off[:, None]                   # planar
            sets.append(("planar", A, Rt @ A + tt[:, None]))
            A = np.vstack([rng.uniform(-1, 1, (2, n)), np.full((1, n), 0.25)]) + off[:, None]  # exactly planar (z const)
            sets.append(("planar_exact", A, Rt @ A + tt[:, None]))
            A = rng.normal(size=(3, 3)) + off[:, None]                          # three points
            sets.append(("three", A, Rt @ A + tt[:, None]))
            A = rng.normal(size=(3, n)) * rng.uniform(0.05, 2, (3, 1)) + off[:, None]
            Bm = A.copy()
            Bm[0] = 2 * off[0] - Bm[0]                                          # mirror image: det H < 0
            sets.append(("mirror", A, Rt @ Bm + tt[:, None]))
            g = np.arange(-2, 3, dtype=float)
            A = np.stack(np.meshgrid(g, g, g)).reshape(3, -1) * 0.1 + off[:, None]  # cube lattice: covariance ~ I
            sets.append(("cube", A, Rt @ A + tt[:, None]))
            A = rng.normal(size=(3, n)) * rng.uniform(0.01, 3, (3, 1)) + off[:, None]
            sets.append(("generic", A, Rt @ A + tt[:, None]))
    return sets


def kabsch_cases(seed=9):
    """(cnt, sa, sb, sab, labels): the sums of kabsch_point_sets and the 500 random sums of test_abi.py."""
    cnt, sa, sb, sab, labels = [], [], [], [], []
    for name, A, B in kabsch_point_sets(seed):
        cnt.append(A.shape[1])
        sa.append(A.sum(1))
        sb.append(B.sum(1))
        sab.append((A @ B.T).reshape(9))
        labels.append(name)
    rng = np.random.default_rng(123)  # tests/test_abi.py's second loop, its draws replayed after the 3000 moments
    for t in range(3000):
        rng.normal(5, 1, 3), rng.normal(0, 1, (3, 3)), rng.uniform(-3, 6)
    for t in range(500):
        n = int(rng.integers(3, 5000))
        A = rng.normal(0, 1, (3, n)) * rng.uniform(0.01, 3, (3, 1))
        if t % 5 == 0:
            A[2] = 0.0
        ang = rng.uniform(-0.5, 0.5, 3)
        Rt = _rot_xyz(ang)
        B = Rt @ A + rng.normal(0, 1, (3, 1))
        cnt.append(n)
        sa.append(A.sum(1))
        sb.append(B.sum(1))
        sab.append((A @ B.T).reshape(9))
        labels.append("random_planar" if t % 5 == 0 else "random")
    return np.array(cnt, np.int64), np.array(sa), np.array(sb), np.array(sab), labels


def _rot_xyz(ang):
    cx, cy, cz = np.cos(ang)
    sx, sy, sz = np.sin(ang)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def p2l_pack(A, b, extra=0.0):
    """The 28 sums solve_p2l reads: the upper triangle of the 6x6 normal matrix row by row, b, one more sum."""
    iu = np.triu_indices(6)
    return np.concatenate([A[iu], b, [extra]])


def p2l_cases(seed=10):
    """(sums (n, 28), labels, theta (n,)): theta = |alpha| of the exact solution (nan where there is none)."""
    rng = np.random.default_rng(seed)
    sums, labels, theta = [], [], []

    def add(A, x, label):
        sums.append(p2l_pack(A, -(A @ x)))
        labels.append(label)
        theta.append(float(np.linalg.norm(x[:3])))

    Dg = np.diag([4.0, 4.0, 4.0, 1.0, 1.0, 1.0])  # exact Cholesky: L = diag(2, 2, 2, 1, 1, 1)
    for k in range(1, 40):
        for sgn in (-1.0, 1.0):
            th = 1e-9 * (1.0 + sgn * 2.0 ** -k)
            for axis in range(3):
                x = np.zeros(6)
                x[axis] = th
                x[3:] = rng.normal(size=3)
                add(Dg, x, "taylor_edge")
    for th in (0.0, 1e-300, 1e-20, 1e-12, 3e-10, 1e-8, 1e-6, 1e-3, 0.1, 0.5, 1.0, 2.0, 3.0, 3.1415):
        for rep in range(6):
            J = rng.normal(size=(40, 6))
            A = J.T @ J
            a = rng.normal(size=3)
            x = np.concatenate([a / np.linalg.norm(a) * th, rng.normal(size=3)])
            add(A, x, "theta")
    for i in range(3000):  # random SPD systems: sin / cos branch, every magnitude of rotation
        J = rng.normal(size=(int(rng.integers(6, 60)), 6)) * rng.uniform(0.05, 3, 6)
        A = J.T @ J
        x = np.concatenate([rng.normal(size=3) * 10.0 ** rng.uniform(-8, 0.3), rng.normal(size=3)])
        add(A, x, "random")
    for k in range(1, 30):  # the pivot test  s > 1e-12 * dmax  on both sides (last pivot s = d exactly)
        for sgn in (-1.0, 1.0):
            d = 1e-12 * (1.0 + sgn * 2.0 ** -k)
            add(np.diag([1.0, 1.0, 1.0, 1.0, 1.0, d]), np.array([1e-3, 0, 0, 0.1, 0.2, 0.3]), "pivot_edge")
            A = np.diag([1.0, 1.0, 1.0, 1.0, 1.0, d])
            A[0, 1] = A[1, 0] = 0.5  # a pivot before the last one is 0.75, exact; the last is still d
            add(A, np.array([0, 1e-4, 0, 0.1, 0.2, 0.3]), "pivot_edge")
    for i in range(30):  # rank-deficient normal matrices: fewer than six independent rows
        J = rng.normal(size=(int(rng.integers(1, 6)), 6))
        add(J.T @ J, rng.normal(size=6), "rank_deficient")
    sums, labels, theta = np.array(sums), labels, np.array(theta)
    nf = []
    for bad in (np.nan, np.inf, -np.inf):
        for pos in (0, 5, 20, 21, 26, 27):
            s = sums[-1].copy()
            s[pos] = bad
            nf.append(s)
    sums = np.concatenate([sums, np.array(nf), np.zeros((1, 28))])
    labels = labels + ["nonfinite"] * len(nf) + ["zero"]
    theta = np.concatenate([theta, np.full(len(nf) + 1, np.nan)])
    return sums, labels, theta


def mat_pairs(seed=11, n=20000):
    """float32 (A, B) for invert3f / mul3f: rotations, generic, singular, near-singular, subnormal, huge, non-finite."""
    rng = np.random.default_rng(seed)
    A = np.concatenate([random_rotation(rng, n // 4), rng.normal(size=(n // 4, 3, 3)) * 10.0 ** rng.uniform(-3, 3, (n // 4, 1, 1)),
                        np.zeros((8, 3, 3))]).astype(np.float32)
    Rk = rng.integers(-3, 4, (200, 3, 3)).astype(np.float32)
    Rk[:, 2] = Rk[:, 0] + Rk[:, 1]  # exactly singular
    Ns = rng.normal(size=(200, 3, 3)).astype(np.float32)
    Ns[:, 2] = Ns[:, 0] + Ns[:, 1] * np.float32(1 + 2 ** -20)  # nearly singular
    spec = rng.normal(size=(60, 3, 3)).astype(np.float32)
    spec[0:10, 0, 0] = np.nan
    spec[10:20, 1, 1] = np.inf
    spec[20:30, 2, 0] = -np.inf
    spec[30:40] *= np.float32(1e-42)  # subnormal
    spec[40:50] *= np.float32(1e30)
    spec[50:60] *= np.float32(1e-20)
    A = np.concatenate([A, Rk, Ns, spec])
    B = A[rng.permutation(len(A))]
    return A, B


# ---------------------------------------------------------------------------------------------- references --
def _mp(M):
    return mpmath.matrix([[mpmath.mpf(float(v)) for v in row] for row in np.asarray(M, np.float64)])


def _np(m):
    return np.array([[float(m[r, c]) for c in range(m.cols)] for r in range(m.rows)])


def mp_svd(M):
    """U, S, V of a float64 3x3 at DIGITS digits: (U (3, 3), S (3,), V (3, 3)) as float64, S descending."""
    with mpmath.workdps(DIGITS):
        U, S, V = mpmath.svd_r(_mp(M))
        return _np(U), np.array([float(s) for s in S]), _np(V).T  # svd_r returns V^T


def mp_polar_reference(M):
    """icp.cpp:215-223 at DIGITS digits: R = V U^T of the SVD of M, then column 2 negated when det R < 0."""
    with mpmath.workdps(DIGITS):
        U, S, Vt = mpmath.svd_r(_mp(M))
        R = Vt.T * U.T
        if mpmath.det(R) < 0:
            for r in range(3):
                R[r, 2] = -R[r, 2]
        return _np(R)


def mp_kabsch(n, sa, sb, sab):
    """rigid_transform_3D.py at DIGITS digits from the same float64 sums: (R, t)."""
    with mpmath.workdps(DIGITS):
        n = mpmath.mpf(int(n))
        ca = mpmath.matrix([mpmath.mpf(float(v)) / n for v in sa])
        cb = mpmath.matrix([mpmath.mpf(float(v)) / n for v in sb])
        H = _mp(np.asarray(sab).reshape(3, 3)) - n * ca * cb.T
        U, S, Vt = mpmath.svd_r(H)
        R = Vt.T * U.T
        if mpmath.det(R) < 0:
            for c in range(3):
                Vt[2, c] = -Vt[2, c]
            R = Vt.T * U.T
        t = -R * ca + cb
        return _np(R), np.array([float(v) for v in t]), _np(H)
