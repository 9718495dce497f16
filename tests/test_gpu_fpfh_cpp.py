"""icp::Engine::computeFPFH / fpfh / matchFeatures / registerGlobal (tests/cpp/test_fpfh.cpp) against the C ABI's output
and against the same calls made through the Python binding, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import fpfh_cases as fc
import mirror
from icp_slam_prototype_amd import binding

pytestmark = pytest.mark.gpu


def test_cpp_engine_equals_c_abi_and_binding():
    p = fc.e2e_pair(n_plane=55, n_clutter=140, normal_radius=0.35)
    src, tgt = p["source"], p["target"]
    ns, nt = src.shape[1], tgt.shape[1]
    radius, n_hyp, seed, max_dist = 0.45, 300, 12, 0.05
    blob = b"".join(np.ascontiguousarray(a, np.float32).tobytes() for a in (src, p["ns"], tgt, p["nt"]))
    raw, _ = mirror.run("test_fpfh", blob, str(ns), str(nt), str(radius), str(n_hyp), str(seed), str(max_dist))
    with binding.Context(0) as c:
        c.set_target(tgt)
        c.set_target_normals(p["nt"])
        c.set_source(src)
        c.set_source_normals(p["ns"])
        c.compute_fpfh(0, radius)
        c.compute_fpfh(1, radius)
        ds, vs = c.get_fpfh(0)
        dt, vt = c.get_fpfh(1)
        m = c.match_features(mutual=True)
        want, rc = c.register_global(n_hyp, seed, max_dist, 0.9)
    assert rc == binding.OK and len(m[0]) >= 10 and want["inliers"] > 0
    rec = np.zeros(len(m[0]), np.dtype([("s", "<i4"), ("t", "<i4"), ("D", "<f4")]))
    rec["s"], rec["t"], rec["D"] = m
    res = binding.GlobalResult()
    res.T[:] = [float(v) for v in want["T"].reshape(16)]
    res.hypothesis, res.n_valid, res.n_matches, res.inliers = want["hypothesis"], want["n_valid"], want["n_matches"], want["inliers"]
    res.sums[:] = [float(v) for v in want["sums"]]
    one = b"".join([ds.tobytes(), vs.astype(np.uint8).tobytes(), dt.tobytes(), vt.astype(np.uint8).tobytes(),
                    np.int32(len(rec)).tobytes(), rec.tobytes(), bytes(res), np.int32(rc).tobytes()])
    assert len(raw) == 2 * len(one)
    assert raw[:len(one)] == raw[len(one):], "Engine and C ABI differ"
    assert raw[:len(one)] == one, "Engine and binding differ"
