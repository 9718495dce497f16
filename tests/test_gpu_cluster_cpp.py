"""icp::Engine::clusterDbscan / clusters (tests/cpp/test_cluster.cpp) against the same calls made by hand through the
Python binding, byte for byte, on config 2's target with clumps of strays."""
import struct

import numpy as np
import pytest

import cluster_model as cm
import mirror
from icp_slam_prototype_amd import binding, cluster, synth

pytestmark = pytest.mark.gpu


def test_cpp_cluster_equals_binding():
    pts, _ = cm.with_clumps(synth.kinect_pair()["target"][:, :30000], n_clumps=10)
    n = pts.shape[1]
    nrm = np.random.default_rng(5).normal(0, 1, pts.shape).astype(np.float32)
    eps, mp, min_size, max_size, largest = 0.03, 6, 20, 0, 0
    blob = struct.pack("<5if", n, mp, min_size, max_size, largest, eps) + pts.tobytes() + nrm.tobytes()
    raw, stdout = mirror.run("test_cluster", blob)
    want = b""
    first = None
    with binding.Context(0) as ctx:
        for call in range(3):
            which = 0 if call == 1 else 1
            if which == 1:
                ctx.set_target(pts)
                if call == 2:
                    ctx.set_target_normals(nrm)
            else:
                ctx.set_source(pts)
            counts = cluster.dbscan(ctx, which, eps, mp, min_size=min_size, max_size=max_size, labels_only=call == 0)
            rec = cluster.clusters(ctx)
            first = first or (counts, rec)
            want += struct.pack("<5i", binding.OK, *counts, rec["n_in"])
            want += b"".join(rec[k].tobytes() for k in ("labels", "core", "count", "nearest_core", "out_index", "sizes", "first"))
            got = ctx.get_target() if which == 1 else ctx.get_source()
            want += struct.pack("<i", got.shape[1]) + got.tobytes()
            assert got.shape[1] == (n if call == 0 else counts[2])
            if call == 2:
                want += ctx.get_target_normals().tobytes()
    want += struct.pack("<2i", binding.E_ARG, binding.E_ARG)
    assert raw == want
    (nc, noise, n_out), rec = first
    model = cm.dbscan(pts, eps, mp, min_size=min_size, max_size=max_size)
    assert (nc, noise, n_out) == (model["n_clusters"], model["n_noise"], model["n_out"]) and nc > 2 and 0 < n_out < n
    assert np.array_equal(rec["labels"], model["labels"])
    assert f"{nc} clusters, {noise} noise, {n_out} kept of {n}" in stdout
