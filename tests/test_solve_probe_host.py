"""CPU-side companion of tests/test_gpu_solve_device.py: the host entry points of the solve probe
(tests/cpp/solve_probe.hip, csrc/solve_impl.h compiled with the library's flags) against the production host code
(binding.solve_*) bit for bit, and against a 50-digit mpmath reference, on the case generators of tests/solve_cases.py.
Also proves that those generators reach every branch the device test is meant to exercise.  No GPU needed."""
from fractions import Fraction

import numpy as np
import pytest

import solve_cases as sc
from icp_slam_prototype_amd import binding, build


@pytest.fixture(scope="module")
def probe():
    build.build()
    binding.load()
    return sc.Probe()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def test_probe_host_equals_production_host_solve(probe):
    """The probe compiles solve_impl.h exactly as libicpk.so does: its host results are the library's, bit for bit."""
    M, _ = sc.reference_cases()
    R = probe.solve_reference(M)
    Rb = np.stack([binding.solve_reference(m) for m in M])
    assert np.array_equal(_bits(R), _bits(Rb))
    cnt, sa, sb, sab, _ = sc.kabsch_cases()
    R, t = probe.solve_kabsch(cnt, sa, sb, sab)
    for i in range(len(cnt)):
        Rb, tb = binding.solve_kabsch(cnt[i], sa[i], sb[i], sab[i].reshape(3, 3))
        assert np.array_equal(_bits(R[i]), _bits(Rb)) and np.array_equal(_bits(t[i]), _bits(tb)), i
    sums, _, _ = sc.p2l_cases()
    ok, R, t = probe.solve_p2l(sums)
    for i in range(len(sums)):
        Rb, tb, rc = binding.solve_point_to_plane(sums[i])
        assert (rc == binding.OK) == bool(ok[i]), i
        if ok[i]:
            assert np.array_equal(_bits(R[i]), _bits(Rb)) and np.array_equal(_bits(t[i]), _bits(tb)), i


def _scaled_det_exact(A):
    """polar3's first-iteration |det|, exactly: the largest entry scaled into [1, 2) by a power of two."""
    amax = float(np.abs(A).max())
    s0 = 2.0 ** -np.floor(np.log2(amax))
    while amax * s0 >= 2.0:
        s0 /= 2
    while amax * s0 < 1.0:
        s0 *= 2
    Q = [[Fraction(float(v) * s0) for v in row] for row in A]
    d = (Q[0][0] * (Q[1][1] * Q[2][2] - Q[1][2] * Q[2][1]) - Q[0][1] * (Q[1][0] * Q[2][2] - Q[1][2] * Q[2][0])
         + Q[0][2] * (Q[1][0] * Q[2][1] - Q[1][1] * Q[2][0]))
    return abs(float(d))


def test_generators_reach_every_branch(probe):
    """With the host probe: polar3 returns false on some cases and true on others, and exactly where the first
    iteration's scaled |det| decides it; svd3 takes its zero-matrix and rank-1 completions; Kabsch takes its reflection
    branch; solve_p2l takes its Taylor branch and refuses on both its pivot test and non-finite sums.

    polar3's later exits (|det| outside [1e-30, 1e30] after the first step, no convergence within 40 steps) are
    asserted NOT to be taken by any finite case past the first test, and cannot be: once |det| >= 1e-7 with the largest
    entry in [1, 2), every singular value lies in [1e-7 / 36, 6], the scaled first step maps each to
    (g s + 1 / (g s)) / 2 with g ~ |det|^(-1/3), so all are >= 1 and <= ~1e6 afterwards (|det| in [1, 1e18]), and the
    scaled Newton iteration then converges quadratically to |det| - 1 <= 1e-5 in under ten steps."""
    A, labels = sc.polar_cases()
    ok, Q = probe.polar3(A)
    assert ok.any() and not ok.all()
    finite = np.isfinite(A).all(axis=(1, 2))
    amax = np.abs(np.where(np.isfinite(A), A, 0)).max(axis=(1, 2))
    in_range = finite & (amax >= 1e-290) & (amax <= 1e290)
    assert not ok[~in_range].any()
    decided = 0
    for i in np.nonzero(in_range)[0]:
        d = _scaled_det_exact(A[i])
        if abs(d - 1e-7) < 1e-13 and labels[i] != "det_switch":
            continue  # the rounded fma chain may land on either side
        assert bool(ok[i]) == (d >= 1e-7), (i, labels[i], d)
        decided += 1
        if ok[i]:
            assert np.abs(Q[i] @ Q[i].T - np.eye(3)).max() < 1e-10, i  # converged (last step: 1e-5 -> 5e-11)
    assert decided > 0.95 * in_range.sum()
    D, side = sc.det_switch_diagonals(np.float64, 50)
    okd, _ = probe.polar3(D)
    assert np.array_equal(okd.astype(bool), side) and side.any() and not side.all()
    U, S, V = probe.svd3(A)
    zero = ~(S[:, 0] > 1e-300)
    rank1 = ~zero & ~((S[:, 1] > 1e-300) & (S[:, 1] > 1e-15 * S[:, 0]))
    assert zero[finite].any() and rank1[finite].any()
    for i in np.nonzero(finite & (zero | rank1))[0]:  # the completions are orthonormal, right-handed
        assert np.abs(U[i] @ U[i].T - np.eye(3)).max() < 1e-12 and np.linalg.det(U[i]) > 0, i
    # Kabsch: the reflection branch (svd3, det(V U^T) < 0 -> last column of V negated)
    cnt, sa, sb, sab, klabels = sc.kabsch_cases()
    ca, cb = sa / cnt[:, None], sb / cnt[:, None]
    H = sab.reshape(-1, 3, 3) - (cnt[:, None] * ca)[:, :, None] * cb[:, None, :]
    okh, _ = probe.polar3(H)
    svd_path = ~((np.linalg.det(H) > 0) & okh.astype(bool))
    Uh, _, Vh = probe.svd3(H)
    reflect = svd_path & (np.linalg.det(Vh @ np.transpose(Uh, (0, 2, 1))) < 0)
    assert reflect.any() and (~svd_path).any()
    assert {klabels[i] for i in np.nonzero(reflect)[0]} >= {"mirror"}
    # solve_p2l: Taylor branch (theta < 1e-9 by a margin far beyond the solve's rounding), pivot test, refusals
    sums, plabels, theta = sc.p2l_cases()
    okp, _, _ = probe.solve_p2l(sums)
    assert ((theta < 1e-9 * (1 - 1e-6)) & okp.astype(bool)).sum() >= 50
    assert ((theta > 1e-9 * (1 + 1e-6)) & okp.astype(bool)).sum() >= 50
    piv = np.array([lab == "pivot_edge" for lab in plabels])
    d = sums[:, 20]  # the last diagonal entry of the normal matrix: the last pivot exactly
    assert np.array_equal(okp[piv].astype(bool), d[piv] > 1e-12)
    assert okp[piv].any() and not okp[piv].all()
    bad = np.array([lab in ("nonfinite", "zero", "rank_deficient") for lab in plabels])
    assert not okp[bad].any()


def _orthonormal(R, tol):
    R = np.asarray(R, np.float64)
    return np.abs(R @ R.T - np.eye(3)).max() < tol and abs(np.linalg.det(R) - 1) < tol


def reference_against_mpmath(M, R, labels):
    """solve_reference's R against icp.cpp:215-223 at 50 digits.  Full-rank moments: the worst deviation is returned
    (the caller bounds it by REFERENCE_MPMATH_BOUND).  Rank-deficient ones (smallest singular value below 1e-6 of the
    largest): orthonormal with det +1, and on the determined subspace R u_i = v_i (or, after icp.cpp:220-223 negated
    column 2, R D u_i = v_i with D = diag(1, 1, -1)).  Returns the worst full-rank deviation."""
    worst = 0.0
    D = np.diag([1.0, 1.0, -1.0])
    for i in range(len(M)):
        if not np.isfinite(M[i]).all() or labels[i] in ("rank0", "huge") or not np.abs(M[i]).max() > 1e-30:
            continue
        Mi = M[i].astype(np.float64)
        U, S, V = sc.mp_svd(Mi)
        Ri = R[i].astype(np.float64)
        assert _orthonormal(Ri, 1e-5), (i, labels[i])
        if S[2] > 1e-6 * S[0]:
            ref = sc.mp_polar_reference(Mi)
            worst = max(worst, float(np.abs(Ri - ref).max()))
            continue
        det_dirs = [k for k in range(3) if S[k] > 1e-6 * S[0]]
        e1 = max(float(np.abs(Ri @ U[:, k] - V[:, k]).max()) for k in det_dirs)
        e2 = max(float(np.abs(Ri @ D @ U[:, k] - V[:, k]).max()) for k in det_dirs)
        assert min(e1, e2) < 1e-5, (i, labels[i], e1, e2)
    return worst


def hardest_reference_cases():
    M, labels = sc.reference_cases()
    keep = [i for i, lab in enumerate(labels) if lab.startswith(("cond", "rank", "diag11eps", "sigmaI", "det_switch"))]
    keep += list(range(len(labels) - 3000, len(labels) - 3000 + 300))  # a slice of the legacy moments
    return M[keep], [labels[i] for i in keep]


def kabsch_against_mpmath(cnt, sa, sb, sab, R, t, labels):
    """Kabsch R, t against rigid_transform_3D.py at 50 digits from the same sums.  Unique rotation (rank(H) >= 2): R
    within 1e-6 and R ca + t = cb to 1e-9 relative to |cb| (test_abi.py's bounds).  Collinear sets (rank 1): R
    orthonormal, det +1, R u0 = v0.  Returns the worst R deviation over the unique cases."""
    worst = 0.0
    for i in range(len(cnt)):
        Rm, tm, Hm = sc.mp_kabsch(cnt[i], sa[i], sb[i], sab[i])
        U, S, V = sc.mp_svd(Hm)
        assert _orthonormal(R[i], 1e-9), (i, labels[i])
        ca, cb = sa[i] / cnt[i], sb[i] / cnt[i]
        assert np.abs(R[i] @ ca + t[i] - cb).max() < 1e-9 * max(1.0, np.abs(cb).max()), (i, labels[i])
        if S[1] > 1e-6 * S[0]:
            worst = max(worst, float(np.abs(R[i] - Rm).max()))
        else:
            assert np.abs(R[i] @ U[:, 0] - V[:, 0]).max() < 1e-6, (i, labels[i])
    return worst


# worst deviations of the host (and, through the bit-for-bit device test, the device) solve from the 50-digit
# reference over these cases.  Reference flavour: measured 3.0e-8 over 2798 moments (the float32 rounding of R),
# so test_abi.py's 2e-5 is tightened to 1e-7 here.  Kabsch: measured 4.2e-7 (10^4 m offsets, where the centring
# cancels), test_abi.py's 1e-6 kept.
REFERENCE_MPMATH_BOUND = 1e-7
KABSCH_MPMATH_BOUND = 1e-6


def test_host_solve_against_mpmath(probe):
    M, labels = hardest_reference_cases()
    worst = reference_against_mpmath(M, probe.solve_reference(M), labels)
    assert worst < REFERENCE_MPMATH_BOUND, worst
    cnt, sa, sb, sab, klabels = sc.kabsch_cases()
    sel = [i for i, lab in enumerate(klabels) if not lab.startswith("random")] + list(range(len(klabels) - 100, len(klabels)))
    R, t = probe.solve_kabsch(cnt[sel], sa[sel], sb[sel], sab[sel])
    worst = kabsch_against_mpmath(cnt[sel], sa[sel], sb[sel], sab[sel], R, t, [klabels[i] for i in sel])
    assert worst < KABSCH_MPMATH_BOUND, worst


def test_host_arithmetic_is_correctly_rounded(probe):
    """The host side of the promise in solve_impl.h: the probe's host sqrt and / are IEEE (numpy's are)."""
    rng = np.random.default_rng(3)
    a = np.abs(rng.normal(size=200000)) * 10.0 ** rng.uniform(-300, 300, 200000)
    b = rng.normal(size=200000) * 10.0 ** rng.uniform(-300, 300, 200000)
    assert np.array_equal(_bits(probe.sqrt(a)), _bits(np.sqrt(a)))
    with np.errstate(all="ignore"):
        assert np.array_equal(_bits(probe.div(a, b)), _bits(a / b))
        af, bf = a.astype(np.float32), b.astype(np.float32)
        assert np.array_equal(_bits(probe.sqrt(af)), _bits(np.sqrt(af)))
        assert np.array_equal(_bits(probe.div(af, bf)), _bits(af / bf))
