"""icp::TsdfVolume::alignSdf / sdfReduce / sdfAssociate / sdfTrace (tests/cpp/test_sdf_track.cpp) against the same calls
made through the Python binding, byte for byte: the pose, the result, every trace entry, the per-pixel cells and the sums
of the room at level 1."""
import struct

import numpy as np
import pytest

import mirror
import sdf_track_cases as sc
import tsdf_cases as tc
from icp_slam_prototype_amd import binding, depth

pytestmark = pytest.mark.gpu


def test_cpp_sdf_track_equals_binding():
    name, iters = "room_l1", 6
    c, t = sc.case(name), tc.case("room")
    v = t["volume"]
    rows, cols = t["frames"][0][0].shape
    blob = struct.pack("<8i", *v["dims"], 255, 0, rows, cols, len(t["frames"]))
    blob += struct.pack("<8f", v["voxel"], *v["origin"], v["trunc"], t["fx"], t["cx"], 0.0)
    for d, P, _ in t["frames"]:
        blob += np.ascontiguousarray(P, np.float64).tobytes() + np.ascontiguousarray(d, np.uint16).tobytes()
    blob += struct.pack("<8i", *c["depth"].shape, c["level"] + 1, c["level"], iters, 6, c["min_weight"], 0)
    blob += struct.pack("<4f", c["fx"], c["cx"], c["max_abs_tsdf"], c["min_normal_cos"]) + c["estimate"].tobytes() + c["depth"].tobytes()
    raw, stdout = mirror.run("test_sdf_track", blob)
    with binding.Context(0) as ctx:
        # the volume fused on the device from the same frames, as the program does (the model's bytes: test_gpu_tsdf.py)
        assert ctx.tsdf_create(dims=v["dims"], voxel=v["voxel"], origin=v["origin"], trunc=v["trunc"]).max_weight == 255
        for d, P, _ in t["frames"]:
            ctx.tsdf_integrate(d, P, fx=t["fx"], cx=t["cx"])
        depth.build_pyramid(ctx, c["depth"], depth.pyramid_params(levels=c["level"] + 1))
        p = sc.sdf_params(name, binding, max_iterations=iters)
        pose, res = binding.align_sdf(ctx, c["estimate"], p)
        trace = binding.sdf_trace(ctx)
        cell, value = binding.sdf_associate(ctx, c["estimate"], p)
        sums, count = binding.sdf_reduce(ctx, c["estimate"], p)
    accepted = int((cell >= 0).sum())
    assert struct.unpack_from("<4i", raw, 0) == (binding.OK, iters, iters, accepted) and accepted == sc.expected(name)["count"] == count
    want = struct.pack("<qd", res.count, res.mean_dist) + pose.tobytes()
    for e in trace:
        want += e["pose"].tobytes() + e["sums"].tobytes() + struct.pack("<q2i", e["count"], e["status"], 0)
    want += cell.tobytes() + value.tobytes() + sums.tobytes() + struct.pack("<q", count)
    assert raw[16:] == want
    assert f"sdf level 1: status 0 after {iters} updates, {res.count} accepted at the last evaluation, {accepted} at the estimate" in stdout
