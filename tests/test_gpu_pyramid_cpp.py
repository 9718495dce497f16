"""icp::Engine::buildDepthPyramid / depthPyramidLevel / backprojectPyramidLevel (tests/cpp/test_pyramid.cpp) against the
same calls made through the Python binding, byte for byte: every level of the pyramid and the target cloud of its last
level with its normals."""
import struct

import numpy as np
import pytest

import mirror
import pyramid_model as pm
from icp_slam_prototype_amd import binding, depth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,levels,smooth", [("room_masked", 3, 0), ("65x131", 4, 1)])
def test_cpp_pyramid_equals_binding(name, levels, smooth):
    img, K = pm.case(name)
    rows, cols = img.shape
    raw, stdout = mirror.run("test_pyramid", np.ascontiguousarray(img).tobytes(), str(rows), str(cols), str(levels),
                             str(K), str(smooth))
    p = depth.pyramid_params(levels=levels, range_cutoff=K)
    b = depth.bilateral_params() if smooth else None
    with binding.Context(0) as ctx:
        shapes = depth.build_pyramid(ctx, img, p, smooth=b)
        got = [depth.pyramid_level(ctx, l) for l in range(levels)]
        n = depth.backproject_level(ctx, levels - 1, which=1, normals_mode=binding.NORMALS_CROSS)
        pts, nrm = ctx.get_target(), ctx.get_target_normals()
    assert struct.unpack_from("<6i", raw, 0) == (binding.OK, n, binding.E_ARG, binding.E_ARG, binding.E_ARG, binding.E_NOT_SET)
    assert n > 50
    want = b"".join(struct.pack("<2i", *s) + g.tobytes() for s, g in zip(shapes, got)) + pts.tobytes() + nrm.tobytes()
    assert raw[24:] == want
    model = pm.pyramid(depth.bilateral_host(img, b) if smooth else img, levels, K)
    assert all(g.tobytes() == m.tobytes() for g, m in zip(got, model))
    assert f"pyramid {rows} x {cols}, {levels} levels: target of {n} points from level {levels - 1}" in stdout
