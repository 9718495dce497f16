"""csrc/solve_impl.h on the device against the same source on the host (tests/cpp/solve_probe.hip, one thread per
case, compiled with the library's flags) and against the production host entry points, on the adversarial cases of
tests/solve_cases.py: exact rank 0 / 1 / 2, repeated singular values, reflections, polar3's 1e-7 switch on both sides,
the 1e-290 / 1e290 guards, subnormal and non-finite entries, Kabsch sums whose centring cancels, solve_p2l's Taylor
switch and pivot test.  solve_impl.h promises host and device agree bit for bit wherever +, -, *, / and sqrt are
correctly rounded on both; the arithmetic sweep checks that premise for the device's sqrt and / directly.

Every comparison is exact (bit patterns) except solve_p2l's R off its Taylor branch, where sin / cos come from ocml on
the device and glibc on the host (bound in test_p2l_device_equals_host)."""
import numpy as np
import pytest

import solve_cases as sc
from icp_slam_prototype_amd import binding, build
from test_solve_probe_host import (KABSCH_MPMATH_BOUND, REFERENCE_MPMATH_BOUND, hardest_reference_cases,
                                   kabsch_against_mpmath, reference_against_mpmath)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    build.build()
    binding.load()
    return sc.Probe()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(dev, host, what):
    """Bit for bit, except the sign of a NaN the operation generated: gfx950 returns the positive quiet NaN
    (0x7ff8...), x86 the negative one (0xfff8...), and IEEE 754 leaves it unspecified.  Where both entries are NaN only
    the sign bit is ignored: NaNs must fall on the same entries and carry the same payload."""
    dev, host = np.ascontiguousarray(dev), np.ascontiguousarray(host)
    bd, bh = _bits(dev), _bits(host)
    if dev.dtype.kind == "f":
        sign = bd.dtype.type(1) << bd.dtype.type(8 * bd.itemsize - 1)
        both_nan = np.isnan(dev) & np.isnan(host)
        bd, bh = np.where(both_nan, bd & ~sign, bd), np.where(both_nan, bh & ~sign, bh)
    diff = bd != bh
    bad = np.nonzero(diff.reshape(len(diff), -1).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} cases differ, first {bad[:5].tolist()}"


def test_polar3_svd3_device_equals_host(probe):
    A, labels = sc.polar_cases()
    okd, Qd = probe.polar3(A, on_device=True)
    okh, Qh = probe.polar3(A)
    assert np.array_equal(okd, okh) and okh.any() and not okh.all()
    _same(Qd[okh == 1], Qh[okh == 1], "polar3 Q")
    Ud, Sd, Vd = probe.svd3(A, on_device=True)
    Uh, Sh, Vh = probe.svd3(A)
    _same(Ud, Uh, "svd3 U")
    _same(Sd, Sh, "svd3 S")
    _same(Vd, Vh, "svd3 V")
    D, side = sc.det_switch_diagonals(np.float64, 50)
    okd, Qd = probe.polar3(D, on_device=True)
    assert np.array_equal(okd.astype(bool), side)


def test_solve_reference_device_equals_host(probe):
    M, labels = sc.reference_cases()
    Rd = probe.solve_reference(M, on_device=True)
    _same(Rd, probe.solve_reference(M), "solve_reference vs probe host")
    _same(Rd, np.stack([binding.solve_reference(m) for m in M]), "solve_reference vs binding")
    Mh, lh = hardest_reference_cases()
    worst = reference_against_mpmath(Mh, probe.solve_reference(Mh, on_device=True), lh)
    assert worst < REFERENCE_MPMATH_BOUND, worst


def test_solve_kabsch_device_equals_host(probe):
    cnt, sa, sb, sab, labels = sc.kabsch_cases()
    Rd, td = probe.solve_kabsch(cnt, sa, sb, sab, on_device=True)
    Rh, th = probe.solve_kabsch(cnt, sa, sb, sab)
    _same(Rd, Rh, "kabsch R")
    _same(td, th, "kabsch t")
    for i in range(len(cnt)):
        Rb, tb = binding.solve_kabsch(cnt[i], sa[i], sb[i], sab[i].reshape(3, 3))
        assert np.array_equal(_bits(Rd[i]), _bits(Rb)) and np.array_equal(_bits(td[i]), _bits(tb)), (i, labels[i])
    # moments that are not sums of real point sets: rank 0 / 1 / 2, reflections, guards, non-finite entries
    A, _ = sc.polar_cases()
    n = len(A)
    rng = np.random.default_rng(12)
    c2 = np.where(np.arange(n) % 2 == 0, 1, rng.integers(3, 10 ** 6, n)).astype(np.int64)
    sa2, sb2 = np.zeros((n, 3)), rng.normal(size=(n, 3))
    Rd, td = probe.solve_kabsch(c2, sa2, sb2, A.reshape(n, 9), on_device=True)
    Rh, th = probe.solve_kabsch(c2, sa2, sb2, A.reshape(n, 9))
    _same(Rd, Rh, "kabsch R (raw moments)")
    _same(td, th, "kabsch t (raw moments)")
    sel = [i for i, lab in enumerate(labels) if not lab.startswith("random")] + list(range(len(labels) - 100, len(labels)))
    Rd, td = probe.solve_kabsch(cnt[sel], sa[sel], sb[sel], sab[sel], on_device=True)
    worst = kabsch_against_mpmath(cnt[sel], sa[sel], sb[sel], sab[sel], Rd, td, [labels[i] for i in sel])
    assert worst < KABSCH_MPMATH_BOUND, worst


def test_invert3f_mul3f_device_equals_host(probe):
    A, B = sc.mat_pairs()
    okd, Id = probe.invert3f(A, on_device=True)
    okh, Ih = probe.invert3f(A)
    assert np.array_equal(okd, okh) and okh.any() and not okh.all()
    _same(Id, Ih, "invert3f")
    _same(probe.mul3f(A, B, on_device=True), probe.mul3f(A, B), "mul3f")


# measured on an MI355X over the 3289 solved cases off the Taylor branch: 28 differ at all, by at most 2.2e-16 (2^-52)
P2L_SINCOS_BOUND = 2.0 ** -52


def test_p2l_device_equals_host(probe):
    """Flag, t and (on the Taylor branch) R bit for bit.  Off the Taylor branch R = I + A1 K + B1 K^2 with A1 =
    sin(th) / th and B1 = (1 - cos(th)) / th^2 from ocml (device) and glibc (host): measured on an MI355X, 28 of the
    3289 solved cases off the Taylor branch differ, none by more than 2^-52 = 2.2e-16 absolute; that is the bound."""
    sums, labels, theta = sc.p2l_cases()
    okd, Rd, td = probe.solve_p2l(sums, on_device=True)
    okh, Rh, th = probe.solve_p2l(sums)
    assert np.array_equal(okd, okh) and okh.any() and not okh.all()
    ok = okh == 1
    _same(td[ok], th[ok], "p2l t")
    taylor = ok & (theta < 1e-9 * (1 - 1e-6))
    assert taylor.sum() >= 50
    _same(Rd[taylor], Rh[taylor], "p2l R (Taylor branch)")
    rest = ok & ~taylor
    diff = np.abs(Rd[rest] - Rh[rest]).max()
    assert diff <= P2L_SINCOS_BOUND, diff


def _f64_inputs(rng, n):
    u = rng.integers(0, 2 ** 63, n, dtype=np.uint64)
    parts = [
        u[: n // 5] & np.uint64((1 << 52) - 1),                                    # subnormals
        u[n // 5: 2 * n // 5],                                                    # random mantissa, every exponent
    ]
    e = np.arange(-1074, 1024)
    p2 = np.ldexp(1.0, e).view(np.uint64)
    near = (p2[:, None].astype(np.int64) + np.arange(-4, 5)[None, :]).reshape(-1)  # powers of 2 (and 4) +- 4 ulp
    parts.append(near[near > 0].astype(np.uint64))
    x = np.abs(u[2 * n // 5: 3 * n // 5].view(np.float64))
    x = x[np.isfinite(x)]
    x = np.ldexp(np.frexp(x)[0], rng.integers(-530, 511, x.size))
    sq = (x * x).view(np.uint64).astype(np.int64)                               # squares of doubles +- 1 ulp
    parts.append((sq[:, None] + np.arange(-1, 2)[None, :]).reshape(-1).astype(np.uint64))
    out = np.concatenate(parts).view(np.float64)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, -1.0, -1e-310, 5e-324, 1.7976931348623157e308])
    return np.concatenate([out[np.isfinite(out) & (out >= 0) | np.isnan(out)], special])


def _f32_inputs(rng, n):
    u = rng.integers(0, 2 ** 31, n, dtype=np.uint32)
    parts = [u[: n // 5] & np.uint32((1 << 23) - 1), u[n // 5: 2 * n // 5]]
    p2 = np.ldexp(np.float32(1), np.arange(-149, 128)).astype(np.float32).view(np.uint32).astype(np.int64)
    near = (p2[:, None] + np.arange(-4, 5)[None, :]).reshape(-1)
    parts.append(near[near > 0].astype(np.uint32))
    x = np.ldexp(np.float32(1) + rng.random(n // 5, dtype=np.float32), rng.integers(-70, 63, n // 5)).astype(np.float32)
    sq = (x * x).view(np.uint32).astype(np.int64)
    parts.append((sq[:, None] + np.arange(-1, 2)[None, :]).reshape(-1).astype(np.uint32))
    parts.append(np.arange(0, 1 << 23, 7, dtype=np.uint32) | np.uint32(127 << 23))  # a dense slice of [1, 2)
    out = np.concatenate(parts).view(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, 1e-45, 3.4028235e38], np.float32)
    return np.concatenate([out, special]).astype(np.float32)


def test_device_arithmetic_is_correctly_rounded(probe):
    """The premise of solve_impl.h's promise: on gfx950 with the library's flags, sqrt(double), double /, sqrtf and
    float / give the host's (IEEE, correctly rounded) bits over ~10^7 inputs each: subnormals, powers of 2 and 4 and
    their neighbours, squares of doubles +- 1 ulp, random mantissas over the whole exponent range, +-0, inf, NaN."""
    rng = np.random.default_rng(2024)
    a = _f64_inputs(rng, 9 * 10 ** 6)
    assert a.size > 9 * 10 ** 6
    with np.errstate(all="ignore"):
        ref = np.sqrt(a)
        h = probe.sqrt(a)
        _same(h, ref, "host sqrt(double)")
        _same(probe.sqrt(a, on_device=True), h, "device sqrt(double)")
        b = a[rng.permutation(a.size)] * np.where(rng.random(a.size) < 0.5, -1.0, 1.0)
        h = probe.div(a, b)
        _same(h, a / b, "host double /")
        _same(probe.div(a, b, on_device=True), h, "device double /")
        f = _f32_inputs(rng, 8 * 10 ** 6)
        h = probe.sqrt(f)
        _same(h, np.sqrt(f), "host sqrtf")
        _same(probe.sqrt(f, on_device=True), h, "device sqrtf")
        g = f[rng.permutation(f.size)] * np.where(rng.random(f.size) < 0.5, np.float32(-1), np.float32(1))
        h = probe.div(f, g)
        _same(h, f / g, "host float /")
        _same(probe.div(f, g, on_device=True), h, "device float /")
