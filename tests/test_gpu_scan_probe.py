"""csrc/block_scan.h at its edges (tests/cpp/scan_probe.hip, one workgroup per call, compiled with the library's flags)
against numpy.cumsum, exactly: the rank and the total of block_excl_scan / block_total for 256 and 1024 threads, called
twice back to back on different data with no barrier in between (the header's contract); scan_rounds around its round
boundaries, in place as int and out of place as long long past 2^31; scan_runs around its run boundaries."""
import ctypes as C

import numpy as np
import pytest

from icp_slam_prototype_amd import build

pytestmark = pytest.mark.gpu

_i32p, _i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)


def _p(a):
    return a.ctypes.data_as(_i64p if a.dtype == np.int64 else _i32p)


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(build.program("scan_probe"))
    for name in ("pair", "rounds_i32", "rounds_i64", "runs"):
        getattr(lib, "probe_scan_" + name).restype = C.c_int
    return lib


def _excl(v, dtype):
    """(the exclusive scan of v, its sum), accumulated in dtype"""
    inc = np.cumsum(v, dtype=dtype)
    return inc - v.astype(dtype), dtype(inc[-1]) if len(v) else dtype(0)


def _block_values(threads):
    rng = np.random.default_rng(threads)
    vals = [np.zeros(threads, np.int32), np.ones(threads, np.int32)]
    for lane in (0, 63, 64, threads - 1):
        v = np.zeros(threads, np.int32)
        v[lane] = 5
        vals.append(v)
    vals.append(rng.integers(0, 8, threads).astype(np.int32))
    return vals


@pytest.mark.parametrize("threads", [256, 1024])
def test_block_scan_and_total_back_to_back(lib, threads):
    vals = _block_values(threads)
    # every value set once as the first and once as the second of two calls that follow each other without a barrier
    for a, b in zip(vals, vals[1:] + vals[:1]):
        out = np.full((6, threads), -1, np.int32)
        assert lib.probe_scan_pair(threads, _p(a), _p(b), _p(out)) == 0
        (ra, sa), (rb, sb) = _excl(a, np.int32), _excl(b, np.int32)
        assert np.array_equal(out[0], ra) and np.array_equal(out[2], rb)
        for row, s in ((1, sa), (3, sb), (4, sa), (5, sb)):  # the total, in every thread
            assert np.array_equal(out[row], np.full(threads, s, np.int32)), row


ROUNDS_M = [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 8192, 8193]


@pytest.mark.parametrize("m", ROUNDS_M)
def test_scan_rounds_int_in_place(lib, m):
    v = np.random.default_rng(m).integers(0, 1025, m).astype(np.int32)
    a, totals = v.copy(), np.full(256, -1, np.int32)
    assert lib.probe_scan_rounds_i32(m, _p(a), _p(totals)) == 0
    want, s = _excl(v, np.int32)
    assert np.array_equal(a, want)
    assert np.array_equal(totals, np.full(256, s, np.int32))


@pytest.mark.parametrize("m", ROUNDS_M)
def test_scan_rounds_int64_out_of_place(lib, m):
    v = np.random.default_rng(m + 1).integers(0, 1025, m).astype(np.int32)
    if m == 8192:  # the TSDF bound: every chunk full, a round stays below 2^31 and the total does not
        v[:] = 3 << 17
    src, out, totals = v.copy(), np.full(m, -1, np.int64), np.full(256, -1, np.int64)
    assert lib.probe_scan_rounds_i64(m, _p(src), _p(out), _p(totals)) == 0
    want, s = _excl(v, np.int64)
    if m == 8192:
        assert s == 3221225472 and s > 2**31
    assert np.array_equal(out, want)
    assert np.array_equal(totals, np.full(256, s, np.int64))


@pytest.mark.parametrize("m", [0, 1, 1023, 1024, 1025, 46080, 46081])
def test_scan_runs(lib, m):
    v = np.random.default_rng(m + 2).integers(0, 1025, m).astype(np.int32)
    a, totals = v.copy(), np.full(1024, -1, np.int32)
    assert lib.probe_scan_runs(m, _p(a), _p(totals)) == 0
    want, s = _excl(v, np.int32)
    assert np.array_equal(a, want)
    assert np.array_equal(totals, np.full(1024, s, np.int32))
