"""icp::TsdfVolume::computeEsdf / esdfPlanes / esdfBox / queryEsdf (tests/cpp/test_tsdf_esdf.cpp) against the same calls
made through the Python binding, byte for byte, on the 37 x 21 x 19 case and on the room."""
import struct

import numpy as np
import pytest

import esdf_cases as ec
import mirror
from icp_slam_prototype_amd import binding

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["odd_r6", "room"])
def test_cpp_esdf_equals_binding(name):
    c = ec.case(name)
    pts = ec.points(name, n=512)
    dims = np.array(c["dims"])
    lo, hi = dims // 3, dims - dims // 4
    e = c["esdf"]
    blob = struct.pack("<12i", *c["dims"], e["min_weight"], e["flags"], pts.shape[1], *lo, *hi)
    blob += np.float32([c["voxel"], *c["origin"], c["trunc"], e["max_distance"]]).tobytes()
    blob += np.ascontiguousarray(c["tsdf"], np.float32).tobytes() + np.ascontiguousarray(c["weight"], np.uint16).tobytes()
    blob += pts.tobytes()
    raw, stdout = mirror.run("test_tsdf_esdf", blob)
    with binding.Context(0) as ctx:
        ec.load(ctx, name)
        counts = binding.esdf_compute(ctx, **e)
        planes, box, q = binding.esdf_get(ctx), binding.esdf_get_box(ctx, lo, hi), binding.esdf_query(ctx, pts)
    want = counts.tobytes() + b"".join(a.tobytes() for a in planes + box) + q["dist"].tobytes() + q["grad"].tobytes() + q["status"].tobytes()
    assert raw == want
    assert np.array_equal(planes[0], ec.model(name)["sq"]) and counts[2] > 100
    assert f"{counts[0]} unknown, {counts[1]} free, {counts[2]} occupied, {counts[3]} far; {pts.shape[1]} points" in stdout
