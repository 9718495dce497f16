"""Global registration on the device (icpk_register_global, K16): the winner, its score and its pose against the numpy
model (tests/fpfh_model.py, scoring through tests/score_model.py) bit for bit, and the end-to-end case: a pair that
icpk_align cannot register from the identity, registered globally and refined to where a refinement from the true pose
ends."""
import numpy as np
import pytest

import fpfh_cases as fc
import fpfh_model as fm
import score_model as sm
from icp_slam_prototype_amd import binding

pytestmark = pytest.mark.gpu

MAX_DIST, EDGE = 0.05, 0.9


@pytest.fixture(scope="module")
def small():
    """a small cluttered pair (about 250 points a side) and its model matches"""
    p = fc.e2e_pair(n_plane=55, n_clutter=140, normal_radius=0.35)
    p["fs"], p["ft"] = fm.fpfh(p["source"], p["ns"], 0.45), fm.fpfh(p["target"], p["nt"], 0.45)
    p["matches"] = fm.match(p["fs"]["desc"], p["fs"]["valid"], p["ft"]["desc"], p["ft"]["valid"], mutual=True)
    return p


def prepared(c, p, r=0.45, mutual=True):
    c.set_target(p["target"])
    c.set_target_normals(p["nt"])
    c.set_source(p["source"])
    c.set_source_normals(p["ns"])
    c.compute_fpfh(0, r)
    c.compute_fpfh(1, r)
    return c.match_features(mutual=mutual)


def same(got, want):
    return (got["hypothesis"] == want["hypothesis"] and got["inliers"] == want["inliers"] and got["n_valid"] == want["n_valid"]
            and got["n_matches"] == want["n_matches"] and got["sums"].tobytes() == want["sums"].tobytes()
            and got["T"].tobytes() == want["T"].tobytes())


@pytest.mark.parametrize("n_hyp,seed,edge", [(1, 5, EDGE), (17, 5, EDGE), (5000, 6, 0.0)])
def test_register_global_equals_the_model(small, n_hyp, seed, edge):
    with binding.Context(0) as c:
        m = prepared(c, small)
        assert np.array_equal(m[0], small["matches"][0]) and np.array_equal(m[1], small["matches"][1])
        assert len(m[0]) >= 10
        outs = [c.register_global(n_hyp, seed, MAX_DIST, edge) for _ in range(3)]
        again = c.score_poses(outs[0][0]["T"], MAX_DIST)
    want = fm.register_global(small["matches"][:2], small["source"], small["target"], n_hyp, seed, MAX_DIST, edge)
    if n_hyp == 5000:
        assert want["n_valid"] > binding.SCORE_MAX_POSES  # the scoring crosses a chunk
    for got, rc in outs:
        assert rc == (binding.OK if want["ok"] else binding.W_TOO_FEW_PAIRS)
        assert same(got, want), (got, want)
    if want["ok"]:
        assert again["inliers"][0] == want["inliers"] and again["sums"][0].tobytes() == want["sums"].tobytes()


def test_fewer_than_three_matches(small):
    p = dict(small)
    p["source"], p["ns"] = np.ascontiguousarray(small["source"][:, :40]), np.ascontiguousarray(small["ns"][:, :40] * 0)
    p["ns"][:, :2] = small["ns"][:, :2]  # two described source points that cannot see each other: no valid source
    with binding.Context(0) as c:
        m = prepared(c, p, mutual=False)
        assert len(m[0]) < 3
        got, rc = c.register_global(64, 1, MAX_DIST, EDGE)
        assert rc == binding.W_TOO_FEW_PAIRS and got["hypothesis"] == -1 and got["inliers"] == 0
        assert got["T"].tobytes() == np.eye(4, dtype=np.float32).tobytes() and got["n_matches"] == len(m[0])
        for bad in (dict(n_hypotheses=0), dict(n_hypotheses=binding.GLOBAL_MAX_HYPOTHESES + 1), dict(max_dist=0.0),
                    dict(max_dist=np.inf), dict(edge_similarity=1.5), dict(edge_similarity=-0.1)):
            with pytest.raises(binding.IcpkError) as e:
                c.register_global(**bad)
            assert e.value.code == binding.E_ARG
        c.set_source(p["source"])
        with pytest.raises(binding.IcpkError) as e:
            c.register_global()
        assert e.value.code == binding.E_NOT_SET


def test_an_empty_cloud_has_too_few_matches(small):
    """an empty target (or source) has no matches: ICPK_W_TOO_FEW_PAIRS with the identity, not an error"""
    empty = np.zeros((3, 0), np.float32)
    for which in (0, 1):
        p = dict(small)
        p["source" if which == 0 else "target"] = empty
        p["ns" if which == 0 else "nt"] = empty
        with binding.Context(0) as c:
            m = prepared(c, p)
            assert len(m[0]) == 0
            got, rc = c.register_global(8, 1, MAX_DIST, EDGE)
            assert rc == binding.W_TOO_FEW_PAIRS and got["n_matches"] == 0 and got["hypothesis"] == -1
            assert got["T"].tobytes() == np.eye(4, dtype=np.float32).tobytes()


def compose(Ta, Tb):
    return np.asarray(Ta, np.float64) @ np.asarray(Tb, np.float64)


def test_end_to_end_global_then_refine():
    """The scene: a room corner with asymmetric clutter (fpfh_cases.e2e_pair, about 2200 points a side), the source
    turned by (25, -40, 60) degrees and shifted by half a metre.  From the identity icpk_align ends in a wrong basin;
    register_global + transform_source + commit_source + align (Kabsch, 20 fixed iterations at max_nn_dist 0.05) must
    end at the pose a refinement from the TRUE pose ends at.

    The allowed gap.  On the CPU the model pipeline (FPFH r = 0.25, mutual matches, 256 hypotheses, seed 1) finds a pose
    0.069 from the truth (largest entry of the 4x4); refined by the oracle's loop it ends 6.91e-6 from the oracle's
    refinement of the true pose (largest entry; both are 8.2e-4 from the truth itself, the noise floor of the pair).
    Two starts in one basin meet only up to the last association flips, so the test allows four times that gap:
    2.8e-5.  Measured on an MI355X: 560 matches, 2111 inliers (truth 2101, from the identity 171), gap 6.91e-6."""
    GAP = 4 * 6.91e-6
    p = fc.e2e_pair()
    src, tgt, Tt = p["source"], p["target"], p["T_true"].astype(np.float32)
    kw = dict(solve=binding.SOLVE_KABSCH, max_iterations=20, fixed_iterations=1)

    def refine(c, T0):
        c.set_source(src)
        c.transform_source(T0[:3, :3], T0[:3, 3])
        c.commit_source()
        T, st, rc = c.align(max_nn_dist=MAX_DIST, **kw)
        assert rc == binding.OK
        return compose(T, T0)

    with binding.Context(0) as c:
        c.set_target(tgt)
        c.set_target_normals(p["nt"])
        c.set_source(src)
        c.set_source_normals(p["ns"])
        truth = c.score_poses(Tt, MAX_DIST)["inliers"][0]
        T_id, _, _ = c.align(max_nn_dist=0.75, **kw)
        from_identity = c.score_poses(T_id, MAX_DIST)["inliers"][0]
        assert from_identity < truth // 2, (from_identity, truth)  # ICP alone does not register this pair
        c.compute_fpfh(0, 0.25)
        c.compute_fpfh(1, 0.25)
        m = c.match_features(mutual=True)
        got, rc = c.register_global(256, 1, MAX_DIST, EDGE)
        assert rc == binding.OK and got["inliers"] > 0.9 * truth, (got["inliers"], truth, len(m[0]))
        A = refine(c, got["T"])
        B = refine(c, Tt)
    gap = np.abs(A - B).max()
    print(f"end to end: {len(m[0])} matches, {got['inliers']} inliers (truth {truth}, from the identity {from_identity}), "
          f"gap {gap:.3e} (allowed {GAP:.3e}), from the truth {np.abs(B - p['T_true']).max():.3e}")
    assert gap <= GAP, gap
