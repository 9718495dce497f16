"""icp::Engine::describeKeypoints / describePoints / describedToCloud / matchDescriptors (tests/cpp/test_brief.cpp)
against the same calls made through the Python binding, byte for byte, on the yaw-24 pair of the textured room."""
import struct

import numpy as np
import pytest

import brief_cases as bc
import mirror
from icp_slam_prototype_amd import binding
from icp_slam_prototype_amd import features as F

pytestmark = pytest.mark.gpu


def test_cpp_brief_equals_binding():
    frames = (bc.frame(None), bc.frame("yaw24"))
    n_hyp, max_dist = 256, 0.05
    blob = struct.pack("<5i", bc.ROWS, bc.COLS, bc.FAST_THRESHOLD, bc.MAX_HAMMING, n_hyp)
    blob += np.float32([bc.FX, bc.CX, max_dist]).tobytes()
    blob += b"".join(np.ascontiguousarray(f[0]).tobytes() for f in frames) + b"".join(np.ascontiguousarray(f[1]).tobytes() for f in frames)
    raw, stdout = mirror.run("test_brief", blob)
    want = b""
    with binding.Context(0) as ctx:
        for which, (bgr, depth) in enumerate(frames):
            ctx.detect_fast(bgr, threshold=bc.FAST_THRESHOLD, capacity=0)
            F.describe_keypoints(ctx, which)
            kp, w, b, v = F.descriptors(ctx, which)
            m = F.described_to_cloud(ctx, which, depth, fx=bc.FX, cx=bc.CX)
            want += struct.pack("<i", len(v)) + kp.tobytes() + w.tobytes() + b.tobytes() + v.tobytes() + struct.pack("<i", m)
        i, j, H, H2 = F.match_descriptors(ctx, max_hamming=bc.MAX_HAMMING, mutual=True, to_clouds=True)
        si, ti, D = F.feature_matches(ctx)
        p = binding.GlobalParams()
        ctx._lib.icpk_default_global_params(p)
        p.n_hypotheses, p.max_dist = n_hyp, max_dist
        r = binding.GlobalResult()
        rc = ctx._lib.icpk_register_global(ctx._h, p, r)
    want += struct.pack("<ii", 1, len(i)) + np.stack([i, j, H, H2], 1).astype(np.int32).tobytes()
    pairs = np.zeros(len(si), np.dtype([("s", "<i4"), ("t", "<i4"), ("D", "<f4")]))
    pairs["s"], pairs["t"], pairs["D"] = si, ti, D
    want += struct.pack("<i", len(si)) + pairs.tobytes() + bytes(r) + struct.pack("<i", rc)
    assert raw == want
    assert len(i) > 300 and rc == binding.OK and r.inliers > 50
    assert f"{len(i)} matches, {len(si)} with cloud points, {r.inliers} inliers" in stdout
