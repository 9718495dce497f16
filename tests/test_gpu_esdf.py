"""The Euclidean distance map of the TSDF volume on the device (K31: icpk_esdf_compute / _get / _get_box / _release)
against the numpy model of tests/esdf_model.py, byte for byte, on every case of tests/esdf_cases.py; the sphere's
analytic bound; the map's lifetime; the refusals."""
import numpy as np
import pytest

import esdf_cases as ec
import esdf_model as em
import tsdf_cases as tc
from icp_slam_prototype_amd import binding
from icp_slam_prototype_amd.tsdf import TsdfVolume

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with binding.Context(0) as c:
        yield c


def equal(got, m):
    return np.array_equal(got[0], m["sq"]) and np.array_equal(got[1], m["cls"]) and got[2].tobytes() == m["dist"].tobytes()


def not_set(call, *a, **kw):
    with pytest.raises(binding.IcpkError) as e:
        call(*a, **kw)
    return e.value.code == binding.E_NOT_SET


def refused(call, *a, **kw):
    with pytest.raises(binding.IcpkError) as e:
        call(*a, **kw)
    return e.value.code == binding.E_ARG


@pytest.mark.parametrize("name", ec.CASES)
def test_device_gives_the_models_bytes(ctx, name):
    c, m = ec.load(ctx, name), ec.model(name)
    counts = binding.esdf_compute(ctx, **c["esdf"])
    first = binding.esdf_get(ctx)
    assert np.array_equal(counts, m["counts"]) and equal(first, m)
    # a sub-box is a slice of the planes: an inner one where the volume has one, and the whole volume
    dims = np.array(c["dims"])
    lo, hi = dims // 3, np.maximum(dims - dims // 4, dims // 3 + 1)
    box = binding.esdf_get_box(ctx, lo, hi)
    sl = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    assert equal(box, dict(sq=m["sq"][sl], cls=m["cls"][sl], dist=m["dist"][sl]))
    assert equal(binding.esdf_get_box(ctx, (0, 0, 0), dims), m)
    only = binding.esdf_get_box(ctx, lo, hi, sq=False, dist=False)
    assert only[0] is None and only[2] is None and np.array_equal(only[1], m["cls"][sl])
    # computing again gives the same bytes, and so does a compute that does not wait for the counts
    assert np.array_equal(binding.esdf_compute(ctx, **c["esdf"]), counts) and equal(binding.esdf_get(ctx), m)
    assert binding.esdf_compute(ctx, counts=False, **c["esdf"]) is None and equal(binding.esdf_get(ctx), m)
    assert binding.esdf_get(ctx, sq=False, cls=False, dist=False) == (None, None, None)


def test_a_smaller_radius_after_a_larger_one(ctx):
    """the buffers of one compute serve the next: nothing of the larger radius is left in them"""
    c = ec.load(ctx, "odd_r6")
    binding.esdf_compute(ctx, max_distance=40 * ec.VOXEL, min_weight=2)
    binding.esdf_compute(ctx, **c["esdf"])
    assert equal(binding.esdf_get(ctx), ec.model("odd_r6"))


def test_sphere_is_within_the_analytic_bound(ctx):
    c = ec.load(ctx, "sphere")
    counts = binding.esdf_compute(ctx, **c["esdf"])
    _, cls, dist = binding.esdf_get(ctx)
    assert counts[3] == 0 and ec.sphere_bounds_hold(dist, cls)


def test_lifetime_what_leaves_the_map_alone_and_what_drops_it():
    room = tc.case("room")
    (d0, P0, _), (d1, P1, _), (d2, P2, _) = room["frames"]
    with binding.Context(0) as ctx:
        assert not_set(binding.esdf_get, ctx) and not_set(binding.esdf_compute, ctx)  # no volume
        binding.esdf_release(ctx)
        vol = TsdfVolume(ctx, fx=tc.ROOM_FX, cx=tc.ROOM_CX, **tc.ROOM_VOLUME)
        assert not_set(binding.esdf_get, ctx) and not_set(binding.esdf_get_box, ctx, (0, 0, 0), (1, 1, 1)) and not_set(binding.esdf_query, ctx, np.zeros((3, 1)))
        vol.integrate(d0, P0)
        vol.integrate(d1, P1)
        n = vol.esdf()
        assert n["occupied"] > 1000 and n["unknown"] > 1000 and n["free"] > 1000 and sum(n.values()) - n["far"] == 64 ** 3
        before = vol.esdf_planes()
        tsdf, weight, _ = vol.planes()
        m = em.distance_map(tsdf, weight, tc.ROOM_VOLUME["voxel"])
        assert equal(before, m) and np.array_equal(list(n.values()), m["counts"])

        def same():
            return all(a.tobytes() == b.tobytes() for a, b in zip(vol.esdf_planes(), before))

        # integration, the signed updates, the extractions, the ray cast and the mesh leave it alone: it is stale
        vol.integrate(d2, P2)
        assert same()
        vol.apply([d2], [(-1, 0, P2)])
        assert same()
        vol.surface()
        assert same()
        vol.raycast(P0, shape=d0.shape)
        assert same()
        vol.mesh()
        assert same()
        # a refused compute leaves it as it was
        assert refused(binding.esdf_compute, ctx, max_distance=0.0) and refused(binding.esdf_compute, ctx, flags=2) and refused(binding.esdf_compute, ctx, min_weight=0)
        assert refused(binding.esdf_compute, ctx, max_distance=0.01) and refused(binding.esdf_compute, ctx, max_distance=65.0)  # R = 0, R = 1040
        assert same()
        # ... and so do the refused boxes and queries
        assert refused(binding.esdf_get_box, ctx, (0, 0, 0), (65, 1, 1)) and refused(binding.esdf_get_box, ctx, (3, 3, 3), (3, 4, 4))
        assert refused(binding.esdf_get_box, ctx, (-1, 0, 0), (1, 1, 1))
        import ctypes as C
        fp = C.POINTER(C.c_float)
        x = np.zeros(4, np.float32).ctypes.data_as(fp)
        assert ctx._lib.icpk_esdf_query(ctx._h, None, x, x, 1, None, None, None, None, None) == binding.E_ARG
        assert ctx._lib.icpk_esdf_query(ctx._h, x, x, x, -1, None, None, None, None, None) == binding.E_ARG
        assert ctx._lib.icpk_esdf_query(ctx._h, None, None, None, 0, None, None, None, None, None) == binding.OK
        assert same()
        # reset, set, shift, release and create drop it
        vol.reset()
        assert not_set(binding.esdf_get, ctx) and not_set(binding.esdf_query, ctx, np.zeros((3, 1)))
        vol.esdf(counts=False)
        vol.set_planes(tsdf, weight)
        assert not_set(binding.esdf_get, ctx)
        vol.esdf()
        assert equal(vol.esdf_planes(), m)
        binding.tsdf_shift(ctx, (0, 0, 0))  # (no shift at all: a no-op)
        assert equal(vol.esdf_planes(), m)
        vol.shift((1, 0, 0))
        assert not_set(binding.esdf_get, ctx)
        vol.esdf(counts=False)
        binding.esdf_release(ctx)
        assert not_set(binding.esdf_get, ctx)
        vol.esdf(counts=False)
        vol.release()
        assert not_set(binding.esdf_get, ctx) and not_set(binding.esdf_compute, ctx)
        ctx.tsdf_create(**{k: tc.ROOM_VOLUME[k] for k in ("dims", "voxel", "origin", "trunc")})
        binding.esdf_compute(ctx)
        ctx.tsdf_create(dims=(8, 8, 8), voxel=0.1, origin=(0, 0, 0), trunc=0.3)
        assert not_set(binding.esdf_get, ctx)
        assert (binding.esdf_compute(ctx, max_distance=0.5) == [512, 0, 0, 512]).all()  # a smaller volume in the larger one's buffers


def test_after_a_shift_a_recompute_equals_the_model_on_the_shifted_planes(ctx):
    c = ec.load(ctx, "room")
    binding.esdf_compute(ctx, **c["esdf"])
    binding.tsdf_shift(ctx, (3, -2, 1))
    tsdf, weight, _ = ctx.tsdf_get()
    assert not np.array_equal(tsdf, c["tsdf"])
    counts = binding.esdf_compute(ctx, **c["esdf"])
    m = em.distance_map(tsdf, weight, c["voxel"], **c["esdf"])
    assert np.array_equal(counts, m["counts"]) and equal(binding.esdf_get(ctx), m)
    assert not np.array_equal(m["sq"], ec.model("room")["sq"])
