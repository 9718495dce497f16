"""The signed update rule of the TSDF volume (K30) without a GPU: icpk_tsdf_voxel_apply -- the host half of
csrc/tsdf_rule.h, the header the kernel includes -- against tests/tsdf_apply_model.py bit for bit; a lone +1 op against
icpk_tsdf_voxel_update; the exact properties of the rule on the model; and the derived bound of a removal.  (The
stand-alone sanitizer program over the op-list validation and the host rule: tests/test_sanitized_programs_host.py.)"""
import numpy as np
import pytest

import tsdf_apply_cases as ac
import tsdf_apply_model as am
import tsdf_cases as tc
from icp_slam_prototype_amd import binding, build


@pytest.fixture(scope="module")
def lib():
    build.build()
    return binding.load()


def params_of(c):
    v = c["volume"]
    return binding.tsdf_params(dims=v["dims"], voxel=v["voxel"], origin=v["origin"], trunc=v["trunc"],
                               max_weight=v.get("max_weight"), flags=binding.TSDF_COLOR if v.get("color") else 0)


def host_state(c):
    n = int(np.prod(c["volume"]["dims"]))
    return np.zeros(n, np.float32), np.zeros(n, np.uint16), np.zeros(n, np.float32) if c["volume"].get("color") else None


@pytest.mark.parametrize("name", ac.BYTE_CASES)
def test_voxel_apply_gives_the_models_bits(lib, name):
    c, m = ac.case(name), ac.model(name)
    f, w, ci = host_state(c)
    counts = binding.tsdf_voxel_apply(params_of(c), c["frames"], c["ops"], f, w, c["intensities"], ci, fx=c["fx"], cx=c["cx"])
    assert counts.tolist() == m["counts"]
    assert f.tobytes() == m["tsdf"].tobytes() and w.tobytes() == m["weight"].tobytes()
    if ci is not None:
        assert ci.tobytes() == m["intensity"].tobytes() and ci.max() > 0
    if name == "fresh_minus":
        assert counts.tolist() == [0, 0, 0] and f.tobytes() == bytes(f.nbytes) and not w.any()
    else:
        assert w.any() and min(counts[1:]) >= 0 and max(counts) > 0


def test_cases_meet_their_events():
    """what the cases were built for, seen on the model"""
    m = ac.model("room")
    assert m["counts"][0] == 0 and m["counts"][1] > 1000      # - on the fresh volume writes nothing
    assert m["counts"][7] == 0 and m["counts"][14] == 0       # every voxel behind the camera, either sign
    assert 0 < m["counts"][6] < m["counts"][5]                # the same frame removed twice: the second finds less
    s = ac.model("saturation")
    n = s["counts"][0]
    assert n > 0 and s["counts"] == [n] * 6 + [0] + [n] * 3  # 1, 2, 2, 2, then 1, 0 and nothing left to remove
    assert s["weight"].max() == 1 and (s["weight"] == 1).sum() == n
    k = ac.model("room_capped")
    # five in against a cap of 3, so the third removal empties the voxels both frames saw and the fourth finds less
    assert k["counts"][4] == k["counts"][0] and 0 < k["counts"][8] < k["counts"][7] and 0 < k["counts"][11] < k["counts"][10]
    assert k["weight"].max() == 1
    assert int(np.prod(ac.case("tail")["volume"]["dims"])) == 2 * 256 + 1
    assert int(np.prod(ac.case("tiny")["volume"]["dims"])) < 256
    for name in ("tiny", "tail"):
        assert min(ac.model(name)["counts"]) > 0


def test_a_lone_plus_op_is_voxel_update(lib):
    for name in ("room_color", "odd", "boundary"):
        c = tc.case(name)
        p = params_of(c)
        f, w, ci = host_state(c)
        g, v, cj = host_state(c)
        for d, P, img in c["frames"]:
            R, t = binding.tsdf_invert_pose(P)
            n1 = binding.tsdf_voxel_update(p, R, t, d, f, w, img, ci, fx=c["fx"], cx=c["cx"])
            n2 = binding.tsdf_voxel_apply(p, [d], [(+1, 0, P)], g, v, None if img is None else [img], cj, fx=c["fx"], cx=c["cx"])
            assert n2.tolist() == [n1]
            assert f.tobytes() == g.tobytes() and w.tobytes() == v.tobytes()
            assert ci is None or ci.tobytes() == cj.tobytes()


def test_plus_then_minus_on_a_fresh_volume_is_the_fresh_volume(lib):
    for name in ("room_color", "odd"):
        c = tc.case(name)
        d, P, img = c["frames"][0]
        f, w, ci = host_state(c)
        n = binding.tsdf_voxel_apply(params_of(c), [d], [(+1, 0, P), (-1, 0, P)], f, w, None if img is None else [img], ci,
                                     fx=c["fx"], cx=c["cx"])
        assert n[0] == n[1] > 0 and f.tobytes() == bytes(f.nbytes) and not w.any()  # (icpk_tsdf_voxel_apply ...)
        assert ci is None or ci.tobytes() == bytes(ci.nbytes)
        # (... and the model)
        vol = am.tsdf_model.Volume(**c["volume"])
        d, P, img = c["frames"][0]
        counts = am.apply(vol, [d], [(+1, 0, P), (-1, 0, P)], c["fx"], c["cx"], None if img is None else [img])
        assert counts[0] == counts[1] > 0
        assert vol.tsdf.tobytes() == bytes(vol.tsdf.nbytes) and not vol.weight.any()  # (+0.0f: no sign bit anywhere)
        assert vol.intensity is None or vol.intensity.tobytes() == bytes(vol.intensity.nbytes)


def test_removal_stays_within_the_derived_bound():
    """+A +B +C then -B against +A +C on the room, by the model: the weight planes are equal and the tsdf planes differ
    by at most ac.REMOVAL_BOUND = (11 + 2.5) EPS (1 + 2^-16) = 8.05e-7 (tsdf_apply_model.error_bound: the worst voxel is
    one that B and one other frame hit -- 2.5 EPS after the second +, then (2 * 2.5 + 5) / 1 + 1 = 11 EPS after -B at
    w = 2; a voxel all three hit carries 2.5, 4.33 and then 11 EPS too; +A +C carries 2.5 EPS).
    Measured on the model for this very case: 1.19e-7 (2 EPS), on 14 846 voxels that differ at all."""
    a, b = ac.model("abcb"), ac.model("ac")
    assert ac.REMOVAL_BOUND == pytest.approx(13.5 * am.EPS, rel=1e-4)
    assert a["weight"].tobytes() == b["weight"].tobytes() and (a["weight"] == 2).sum() > 1000
    diff = np.abs(a["tsdf"].astype(np.float64) - b["tsdf"].astype(np.float64))
    print(f"removal: max |diff| {diff.max():.3g} ({diff.max() / am.EPS:.2f} EPS) on {(diff > 0).sum()} voxels that differ, "
          f"bound {ac.REMOVAL_BOUND:.3g}")
    assert 0 < diff.max() <= ac.REMOVAL_BOUND


def test_error_bound_recurrence():
    assert am.error_bound([+1]) == 0 and am.error_bound([+1, -1]) == 0 and am.error_bound([-1]) is None
    assert am.error_bound([+1, +1]) == pytest.approx(2.5, rel=1e-4)
    assert am.error_bound([+1, +1, -1]) == pytest.approx(11, rel=1e-4)
    assert am.error_bound([+1, +1, +1, -1]) == pytest.approx(11, rel=1e-4)
    assert am.worst_error_bound([(+1, "a"), (+1, "b"), (+1, "c"), (-1, "b")]) == pytest.approx(11, rel=1e-4)
