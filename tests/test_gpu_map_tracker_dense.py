"""icp::MapTracker with dense = true (icp_map.hpp, tests/cpp/test_map_tracker_dense.cpp) against the same frames
through the binding, call for call: status, iterations, T and the point list after every fold must be bit equal."""
import struct

import numpy as np
import pytest

import mirror
from icp_slam_prototype_amd import binding
from test_gpu_map import I3, P5, inv3_pose, live_frames, mul3f

pytestmark = pytest.mark.gpu

MAX_ITER, THR, FACTOR, SEED = 10, 1e-5, 40, 17


def test_dense_map_tracker_cpp_matches_the_binding(oracle):
    frames, kp = live_frames()
    rows, cols = frames[0].shape
    parts = [struct.pack("<6ifQ", rows, cols, len(frames), MAX_ITER, kp.shape[0], FACTOR, THR, SEED)]
    for d in frames:
        parts.append(d.tobytes())
    parts.append(kp.tobytes())
    raw, _ = mirror.run("test_map_tracker_dense", b"".join(parts), timeout=None)
    off = 0
    with binding.Context(0) as ctx:
        ctx.set_subsample(FACTOR, SEED)
        ctx.map_reset()
        Rcam, pcam, lastR, lastT = I3.copy(), P5.copy(), I3.copy(), np.zeros(3, np.float32)
        iters = []
        for f in range(1, len(frames)):
            data, previous = frames[f], frames[f - 1]
            if ctx.map_size(binding.MAP_POINTS) == 0:  # the seed (icp.cpp:47-68), as MapTracker makes it
                kprev = oracle.transform_points(binding.backproject_keypoints(previous, kp)[0], I3, P5)
                ctx.map_update_points(binding.MAP_ADD_CLOUD, kprev, 180)
                ctx.backproject(previous, which=1)
                ctx.transform_target(I3, P5)
                ctx.map_set_points(binding.MAP_FROM_TARGET)
            ctx.backproject(data, which=0)
            ctx.transform_source(Rcam, pcam)
            ctx.commit_source()
            params = binding.default_params(max_nn_dist=0.75, max_iterations=MAX_ITER, threshold=THR, solve=0,
                                            last_rotation=lastR, last_translation=lastT)
            T, st, rc = ctx.align_to_map_dense(params, delta=25)
            trace = ctx.get_trace(MAX_ITER)
            for it in trace:
                Rcam = mul3f(Rcam, inv3_pose(it["R"]))
                pcam = (pcam - it["t"]).astype(np.float32)
            lastT = (-T[:3, 3]).astype(np.float32)
            if rc != binding.W_TOO_FEW_PAIRS:
                lastR = I3.copy()
            crc, citer, cpairs, nk, npt = struct.unpack_from("<5i", raw, off)
            off += 20
            cT = np.frombuffer(raw, np.float32, 16, off).reshape(4, 4)
            off += 64
            cpts = np.frombuffer(raw, np.float32, 3 * npt, off).reshape(3, npt)
            off += 12 * npt
            assert (crc, citer, cpairs) == (rc, st.iterations, st.final_pairs), f
            assert nk == ctx.map_size(binding.MAP_KEYPOINTS)
            assert np.array_equal(cT.view(np.uint32), T.view(np.uint32)), f
            assert np.array_equal(cpts.view(np.uint32), ctx.map_get_list(binding.MAP_POINTS).view(np.uint32)), f
            iters.append(st.iterations)
    assert off == len(raw)
    assert max(iters) > 0
