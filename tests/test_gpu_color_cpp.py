"""icp::Engine's colored ICP surface (tests/cpp/test_color.cpp) on the flat wall against the same calls made through
the Python binding, bit for bit."""
import struct

import numpy as np
import pytest

import color_model as cm
import mirror
from icp_slam_prototype_amd import binding

pytestmark = pytest.mark.gpu


def test_cpp_engine_equals_binding():
    p = cm.wall_pair()
    src, tgt = p["source"], p["target"]
    ns, nt = src.shape[1], tgt.shape[1]
    cloud = (src, p["source_intensity"], tgt, p["target_normals"], p["target_intensity"])
    blob = b"".join(np.ascontiguousarray(a, np.float32).tobytes() for a in cloud)
    raw, _ = mirror.run("test_color", blob, str(ns), str(nt), str(cm.WALL_RADIUS), str(cm.WALL_MIN_NB),
                        str(cm.LAMBDA), str(cm.WALL_MAX_DIST), str(cm.WALL_ITER))
    assert len(raw) == 28 + 64
    head = struct.unpack_from("<7i", raw, 0)
    T = np.frombuffer(raw, np.float32, 16, 28).reshape(4, 4)
    with binding.Context(0) as c:
        c.set_target(tgt)
        c.set_target_normals(p["target_normals"])
        c.set_source(src)
        c.set_target_colors(p["target_intensity"])
        c.set_source_colors(p["source_intensity"])
        c.estimate_target_color_gradients(cm.WALL_RADIUS, cm.WALL_MIN_NB)
        c.set_colored(True, cm.LAMBDA)
        want, st, rc = c.align(solve=binding.SOLVE_POINT_TO_PLANE, max_iterations=cm.WALL_ITER, fixed_iterations=1,
                               max_nn_dist=cm.WALL_MAX_DIST)
    assert head == (binding.W_DEGENERATE, rc, st.iterations, st.final_pairs, binding.E_ARG, binding.E_ARG, binding.E_NOT_SET)
    assert rc == 0 and st.iterations == cm.WALL_ITER
    assert T.tobytes() == want.tobytes()
    er, et = cm.pose_errors(T, p["T_true"])
    assert er <= 2 * cm.WALL_MEASURED[0] and et <= 2 * cm.WALL_MEASURED[1]
