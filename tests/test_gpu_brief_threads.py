"""K32 under threads and on a context with a history: eight threads with a context each, and one context that has run
other families before and between, give the bytes of a fresh context's serial run."""
import threading
import traceback

import numpy as np
import pytest

import brief_cases as bc
from icp_slam_prototype_amd import binding, synth
from icp_slam_prototype_amd import features as F

pytestmark = pytest.mark.gpu


def brief_bytes(ctx, variant=0):
    """the whole surface of the feature: both describe routes, the slots' round trip, the clouds with their maps, the
    match with K16's list, and the pose"""
    out = []
    shape = bc.IMAGE_SHAPES[3 + variant % 2]
    img = bc.random_image(*shape, 3 if variant % 2 else 1, seed=variant)
    kp = bc.border_keypoints(*shape, 257, seed=variant)
    F.describe_points(ctx, 1, img, kp, upright=bool(variant & 2))
    stored = F.descriptors(ctx, 1)
    out += list(stored)
    bgr_a, depth_a = bc.frame(None)
    bgr_b, depth_b = bc.frame(bc.POSES[variant % 3][0])
    for which, (bgr, depth) in enumerate(((bgr_a, depth_a), (bgr_b, depth_b))):
        ctx.detect_fast(bgr, threshold=bc.FAST_THRESHOLD, capacity=0)
        F.describe_keypoints(ctx, which)
        out.append(np.int32(F.described_to_cloud(ctx, which, depth, fx=bc.FX, cx=bc.CX)))
        out += list(F.descriptors(ctx, which)) + [F.descriptor_cloud_map(ctx, which)]
    out += [ctx.get_source(), ctx.get_target()]
    out += list(F.match_descriptors(ctx, max_hamming=bc.MAX_HAMMING, ratio=(9, 10) if variant & 1 else None, to_clouds=True))
    out += list(F.feature_matches(ctx))
    g, rc = ctx.register_global(n_hypotheses=128, seed=variant, max_dist=0.05)
    out += [g["T"], np.int64(g["inliers"]), np.int32(g["hypothesis"]), np.int32(rc)]
    F.set_descriptors(ctx, 0, *stored)  # a stored slot against a live one
    out += list(F.match_descriptors(ctx, max_hamming=80, mutual=False))
    return b"".join(np.asarray(a).tobytes() for a in out)


@pytest.fixture(scope="module")
def serial():
    out = []
    for v in range(4):
        with binding.Context(0) as ctx:
            out.append(brief_bytes(ctx, v))
    assert len(set(out)) == 4
    return out


def test_eight_threads_with_a_context_each_give_the_serial_bytes(serial):
    got, errors = [None] * 8, []

    def work(k):
        try:
            with binding.Context(0) as ctx:
                got[k] = brief_bytes(ctx, k % 4)
        except Exception:  # noqa: BLE001 -- reported below, with the thread's traceback
            errors.append(traceback.format_exc())

    threads = [threading.Thread(target=work, args=(k,)) for k in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[0]
    for k in range(8):
        assert got[k] == serial[k % 4], k


def test_a_reused_context_gives_a_fresh_contexts_bytes(serial):
    p = synth.kinect_pair(rows=60, cols=80, seed=3)
    with binding.Context(0) as ctx:
        # other families first: an alignment, normals + FPFH + K16's own match list, a FAST detection with its cloud
        ctx.set_target(p["target"])
        ctx.set_source(p["source"])
        T, st, rc = ctx.align(max_iterations=4)
        assert rc == 0
        ctx.estimate_target_normals(0.2)
        ctx.estimate_source_normals(0.2)
        ctx.compute_fpfh(0, 0.3)
        ctx.compute_fpfh(1, 0.3)
        ctx.match_features(mutual=True)
        bgr, depth = bc.frame("roll30")
        ctx.detect_fast(bgr)
        ctx.detected_to_cloud(depth, which=1, fx=bc.FX, cx=bc.CX)
        for v in (2, 0, 3, 1, 2):  # growing and shrinking slots, the cases in another order, one of them twice
            assert brief_bytes(ctx, v) == serial[v], v
            if v == 0:  # ... and the other families in between leave it and are left by it
                ctx.set_target(p["target"])
                ctx.set_source(p["source"])
                T2, st2, rc2 = ctx.align(max_iterations=4)
                assert rc2 == 0 and T2.tobytes() == T.tobytes()
