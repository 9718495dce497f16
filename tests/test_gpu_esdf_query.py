"""THE QUERY RULE on the device (K31: icpk_esdf_query) against its numpy restatement in tests/esdf_model.py, byte for
byte: random points in and around the volume, points on cell borders, points just below dims - 1, a NaN, n = 0 and
n = 1; and the origin a shifted volume is read with."""
import numpy as np
import pytest

import esdf_cases as ec
import esdf_model as em
from icp_slam_prototype_amd import binding

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with binding.Context(0) as c:
        yield c


def same(got, want):
    return np.array_equal(got["status"], want["status"]) and got["dist"].tobytes() == want["dist"].tobytes() and \
        got["grad"].tobytes() == want["grad"].tobytes()


@pytest.mark.parametrize("name", ["odd_r6", "odd_r1", "line_x", "line_z", "dim_x", "one", "empty", "corner", "room", "room_flag", "sphere"])
def test_query_gives_the_models_bytes(ctx, name):
    c, m = ec.load(ctx, name), ec.model(name)
    binding.esdf_compute(ctx, counts=False, **c["esdf"])
    pts = ec.points(name)  # 4096 random points, 256 + 256 on cell borders, 64 at the last cell's end, g = 0, g = dims - 1, a NaN
    got = binding.esdf_query(ctx, pts)
    want = em.query(m["sq"], m["cls"], c["dims"], c["voxel"], c["origin"], m["R"], pts)
    assert same(got, want)
    assert got["status"][-1] == em.Q_OUTSIDE and got["dist"][-1] == 0 and not got["grad"][:, -1].any()  # the NaN
    if min(c["dims"]) >= 2:
        assert (got["status"] != em.Q_OUTSIDE).sum() > 1000 and (got["status"] == em.Q_OUTSIDE).sum() > 100
    else:
        assert (got["status"] == em.Q_OUTSIDE).all()
    # n = 0 and n = 1
    none = binding.esdf_query(ctx, pts[:, :0])
    assert none["dist"].shape == (0,) and none["grad"].shape == (3, 0)
    k = int(np.flatnonzero(got["status"] != em.Q_OUTSIDE)[0]) if min(c["dims"]) >= 2 else 0
    assert same(binding.esdf_query(ctx, pts[:, k:k + 1]), {key: v[..., k:k + 1] for key, v in want.items()})


def test_every_status_is_seen(ctx):
    """the room has unknown voxels wherever it has far ones; the corner case is known everywhere and far in places"""
    seen = set()
    for name in ("room", "corner"):
        c = ec.load(ctx, name)
        binding.esdf_compute(ctx, **c["esdf"])
        seen |= set(int(s) for s in np.unique(binding.esdf_query(ctx, ec.points(name))["status"]))
    assert seen == {0, em.Q_FAR, em.Q_UNKNOWN, em.Q_FAR | em.Q_UNKNOWN, em.Q_OUTSIDE}


def test_after_a_shift_the_query_reads_the_current_origin(ctx):
    c = ec.load(ctx, "room")
    binding.esdf_compute(ctx, **c["esdf"])
    binding.tsdf_shift(ctx, (3, -2, 1))
    p, total = binding.tsdf_get_params(ctx)
    assert list(total) == [3, -2, 1] and tuple(p.origin) != tuple(np.float32(c["origin"]))
    tsdf, weight, _ = ctx.tsdf_get()
    binding.esdf_compute(ctx, **c["esdf"])
    m = em.distance_map(tsdf, weight, c["voxel"], **c["esdf"])
    pts = ec.points("room")
    got = binding.esdf_query(ctx, pts)
    assert same(got, em.query(m["sq"], m["cls"], c["dims"], c["voxel"], tuple(p.origin), m["R"], pts))
    assert not same(got, em.query(m["sq"], m["cls"], c["dims"], c["voxel"], c["origin"], m["R"], pts))
