"""icp::Engine::bilateralDepthImage / backprojectSmoothed (tests/cpp/test_bilateral.cpp) against the same calls made
through the Python binding, byte for byte: the smoothed image (filtered in place there) and the smoothed target cloud
with its normals."""
import struct

import numpy as np
import pytest

import bilateral_model as bm
import mirror
from icp_slam_prototype_amd import binding, depth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["room_masked", "radius_6"])
def test_cpp_bilateral_equals_binding(name):
    img, fields = bm.case(name)
    p = depth.bilateral_params(**fields)
    rows, cols = img.shape
    raw, stdout = mirror.run("test_bilateral", np.ascontiguousarray(img).tobytes(), str(rows), str(cols), str(p.radius),
                             repr(p.sigma_space), repr(p.sigma_range), str(p.range_cutoff))
    with binding.Context(0) as ctx:
        smooth = depth.bilateral_depth_image(ctx, img, p)
        n = depth.backproject_smoothed(ctx, img, which=1, normals_mode=binding.NORMALS_CROSS, params=p)
        pts, nrm = ctx.get_target(), ctx.get_target_normals()
    assert struct.unpack_from("<4i", raw, 0) == (binding.OK, n, binding.E_ARG, binding.E_ARG) and n > 1000
    want = smooth.tobytes() + pts.tobytes() + nrm.tobytes()
    assert len(want) == 2 * rows * cols + 24 * n and raw[16:] == want
    assert smooth.tobytes() == bm.bilateral(img, *depth.bilateral_tables(p)).tobytes()
    assert f"bilateral {rows} x {cols}, radius {p.radius}: smoothed target of {n} points" in stdout
