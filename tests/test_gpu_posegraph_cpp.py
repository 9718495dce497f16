"""icp::PoseGraph (tests/cpp/test_pose_graph.cpp) on case B against the same call made through the Python binding, byte
for byte."""
import struct

import numpy as np
import pytest

import mirror
import posegraph_cases as pc
from icp_slam_prototype_amd import binding

pytestmark = pytest.mark.gpu


def test_cpp_pose_graph_equals_binding():
    c = pc.case("B")
    n, m = len(c["poses"]), len(c["edges"])
    parts = [struct.pack("<4id", n, m, 0, 0, 0.0),
             np.ascontiguousarray(c["poses"], np.float64).tobytes()]
    for s, t, T, info, u in c["edges"]:
        parts.append(struct.pack("<4i", s, t, int(u), 0))
        parts.append(np.ascontiguousarray(T, np.float64).tobytes())
        parts.append(np.ascontiguousarray(info, np.float64).tobytes())
    raw, stdout = mirror.run("test_pose_graph", b"".join(parts))
    assert stdout.count("node ") == n
    assert len(raw) == 24 + 24 + 128 * n + 16 * m + m
    status, iterations, accepted, pcg, n_pruned, _ = struct.unpack_from("<6i", raw, 0)
    costs = np.frombuffer(raw, np.float64, 3, 24)
    with binding.Context(0) as ctx:
        P, res, w, chi2, pruned, rc = ctx.pose_graph_optimize(c["poses"], c["edges"])
    assert (status, iterations, accepted, pcg, n_pruned) == (rc, res.iterations, res.accepted, res.pcg_iterations, res.n_pruned)
    assert costs.tobytes() == np.array([res.initial_cost, res.final_cost, res.final_lambda]).tobytes()
    o = 48
    assert raw[o:o + 128 * n] == P.tobytes()
    o += 128 * n
    assert raw[o:o + 8 * m] == w.tobytes() and raw[o + 8 * m:o + 16 * m] == chi2.tobytes()
    assert raw[o + 16 * m:] == pruned.astype(np.uint8).tobytes()
    # the printed poses are the same numbers
    first = [float(v) for v in stdout.splitlines()[0].split(":")[1].split()]
    assert np.array_equal(np.array(first), P[0].reshape(16)[:12])
