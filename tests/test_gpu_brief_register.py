"""K32 end to end: features.FrameRegistrar on the three pose pairs of the textured room at 240 x 320 -- the device's
match list against the numpy model's, byte for byte, and the pose after the icpk_align refinement against the same
refinement started at the true pose.

Measured on an MI355X (register_global: 4096 hypotheses, max_dist 0.05; refinement: 30 Kabsch iterations over the pairs
within 0.05 m of the dense clouds; errors against the truth as translation / rotation; `inliers` are the key-point cloud's
points within max_dist under the winning pose; no bound is asserted on the RANSAC's own pose):
    pair     kept   in K16's list  inliers  RANSAC pose error    refined             refined from the truth
    yaw24     789    789           1717     14.6 mm / 0.64 deg   7.0 mm / 0.00 deg   6.5 mm / 0.02 deg
    yaw48     600    600           1162     16.8 mm / 0.38 deg   3.6 mm / 0.04 deg   3.5 mm / 0.03 deg
    roll30   1179   1179           2144      8.6 mm / 0.30 deg   4.5 mm / 0.02 deg   3.9 mm / 0.12 deg
The yaw-48 pair through projective frame-to-frame alignment from the identity (ProjectiveOdometry, the loop ModelTracker
runs against a view) ends 2891 mm / 86.7 degrees from the truth: it is outside that loop's basin, and inside this one."""
import numpy as np
import pytest

import brief_cases as bc
from icp_slam_prototype_amd import binding
from icp_slam_prototype_amd import features as F
from icp_slam_prototype_amd.features import FrameRegistrar
from icp_slam_prototype_amd.odometry import ProjectiveOdometry

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [p[0] for p in bc.POSES])
def test_frame_registrar_on_the_textured_room(name):
    bgr_a, depth_a = bc.frame(None)
    bgr_b, depth_b = bc.frame(name)
    T_true = bc.true_pose(name)
    with binding.Context(0) as ctx:
        reg = FrameRegistrar(ctx, fx=bc.FX, cx=bc.CX, fast_threshold=bc.FAST_THRESHOLD, max_hamming=bc.MAX_HAMMING, max_dist=0.05)
        out = reg.register(bgr_a, depth_a, bgr_b, depth_b)
        assert out["status"] == binding.OK and out["refine_status"] >= 0
        # the device's match list is the model's, byte for byte (the register call left slots and list in place... the
        # refinement replaced the clouds, so the list is read from a second, unrefined run)
        reg2 = FrameRegistrar(ctx, fx=bc.FX, cx=bc.CX, fast_threshold=bc.FAST_THRESHOLD, max_hamming=bc.MAX_HAMMING, max_dist=0.05,
                              refine=False)
        out2 = reg2.register(bgr_a, depth_a, bgr_b, depth_b)
        assert np.array_equal(out2["T"], out["T_global"]) and out2["inliers"] == out["inliers"]
        want = bc.model_pair(name)
        got = F.match_descriptors(ctx, reg2.match)
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want["matches"]))
        for which, side in enumerate((want["src"], want["tgt"])):
            assert all(g.tobytes() == w.tobytes() for g, w in zip(F.descriptors(ctx, which), side))
        assert out["matches"] == len(want["matches"][0]) and out["cloud_matches"] <= out["matches"]
        # the reference: the same refinement started at the true pose
        T_ref, st_ref, rc_ref = reg.refine_from(T_true, depth_a, depth_b)
        assert rc_ref >= 0
    e_global, e_ref, e = bc.pose_error(out["T_global"], T_true), bc.pose_error(T_ref, T_true), bc.pose_error(out["T"], T_true)
    print(f"{name}: kept {out['matches']}, in K16's list {out['cloud_matches']}, inliers {out['inliers']}; RANSAC pose error "
          f"{1e3 * e_global[0]:.1f} mm / {e_global[1]:.2f} deg; refined {1e3 * e[0]:.1f} mm / {e[1]:.2f} deg; refined from the "
          f"truth {1e3 * e_ref[0]:.1f} mm / {e_ref[1]:.2f} deg")
    assert e[0] <= 1.5 * e_ref[0] + 1e-3 and e[1] <= 1.5 * e_ref[1] + 0.05


def test_projective_alignment_from_identity_on_the_yaw48_pair_is_reported():
    """what this buys: the projective frame-to-frame loop from the identity on the widest pair.  Reported, not bounded."""
    _, depth_a = bc.frame(None)
    _, depth_b = bc.frame("yaw48")
    T_true = bc.true_pose("yaw48")
    with binding.Context(0) as ctx:
        odo = ProjectiveOdometry(ctx, fx=bc.FX, cx=bc.CX)
        odo.track(depth_a)
        try:
            pose = odo.track(depth_b)
            e = bc.pose_error(np.linalg.inv(pose), T_true)
            print(f"yaw48, projective frame-to-frame from identity: {1e3 * e[0]:.0f} mm / {e[1]:.1f} deg from the truth")
        except (RuntimeError, binding.IcpkError) as err:
            print(f"yaw48, projective frame-to-frame from identity: lost ({err})")
