"""The distance map (K31) on a context with a history -- an alignment, a ray cast, a mesh and an SDF-tracked frame
behind it -- gives a fresh context's bytes, and leaves what those calls left; two threads with a context each give their
serial bytes."""
import threading
import traceback

import numpy as np
import pytest

import esdf_cases as ec
import tsdf_cases as tc
from icp_slam_prototype_amd import binding, depth as depth_front, synth
from icp_slam_prototype_amd.tsdf import TsdfVolume

pytestmark = pytest.mark.gpu

NAMES = ("odd_r6", "room_flag")


def esdf_bytes(ctx, name):
    """the whole surface of the feature on one case: counts, planes, a box and a query"""
    c = ec.load(ctx, name)
    counts = binding.esdf_compute(ctx, **c["esdf"])
    dims = np.array(c["dims"])
    out = [counts, *binding.esdf_get(ctx), *binding.esdf_get_box(ctx, dims // 3, dims - dims // 4)]
    q = binding.esdf_query(ctx, ec.points(name, n=512))
    return b"".join(a.tobytes() for a in out + [q["dist"], q["grad"], q["status"]])


@pytest.fixture(scope="module")
def fresh():
    out = {}
    for name in NAMES:
        with binding.Context(0) as ctx:
            out[name] = esdf_bytes(ctx, name)
    return out


def test_a_reused_context_gives_a_fresh_contexts_bytes(fresh):
    room = tc.case("room")
    (d0, P0, _), (d1, P1, _), _ = room["frames"]
    p = synth.kinect_pair(rows=60, cols=80, seed=3)
    with binding.Context(0) as ctx:
        ctx.set_target(p["target"])
        ctx.set_source(p["source"])
        T, st, rc = ctx.align(max_iterations=4)
        assert rc == 0
        vol = TsdfVolume(ctx, fx=tc.ROOM_FX, cx=tc.ROOM_CX, **tc.ROOM_VOLUME)
        vol.integrate(d0, P0)
        assert vol.raycast(P0, shape=d0.shape)["n_hits"] > 1000
        assert vol.mesh()["n_triangles"] > 1000
        depth_front.build_pyramid(ctx, d1, depth_front.pyramid_params(levels=1))
        _, res = binding.align_sdf(ctx, P0, fx=tc.ROOM_FX, cx=tc.ROOM_CX, max_iterations=3)
        assert res.count > 1000
        trace = binding.sdf_trace(ctx)
        source = ctx.get_source().tobytes()
        # the map of the volume those calls read, then the cases in both orders
        vol.esdf()
        held = [a.tobytes() for a in vol.esdf_planes()]
        assert ctx.get_source().tobytes() == source and len(binding.sdf_trace(ctx)) == len(trace)  # (it touched neither)
        ray = ctx.tsdf_get_raycast()
        vol.esdf(max_distance=1.0, counts=False)
        assert all(np.array_equal(a, b) for a, b in zip(ray.values(), ctx.tsdf_get_raycast().values()) if isinstance(a, np.ndarray))
        vol.esdf()
        assert [a.tobytes() for a in vol.esdf_planes()] == held
        for name in NAMES + NAMES[::-1]:
            assert esdf_bytes(ctx, name) == fresh[name], name


def test_two_threads_with_a_context_each_give_their_serial_bytes(fresh):
    got, errors = {}, []

    def body(name):
        try:
            with binding.Context(0) as ctx:
                for _ in range(3):
                    got[name] = esdf_bytes(ctx, name)
        except Exception:  # noqa: BLE001 (reported below, with its trace)
            errors.append(traceback.format_exc())

    threads = [threading.Thread(target=body, args=(name,)) for name in NAMES]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert got == fresh
