"""The shift rule and the leaving list (K23) on the numpy models alone: the surface list before a shift is the leaving
list plus the list of the shifted volume mapped back, exactly and disjointly; the origin comes back bit for bit; the
rounding of TsdfVolume.follow."""
import numpy as np
import pytest

import tsdf_cases as tc
import tsdf_shift_cases as sc
import tsdf_shift_model as sm
from icp_slam_prototype_amd import binding
from icp_slam_prototype_amd.tsdf import TsdfVolume

CASES = sc.CASES
shifts = sc.named_shifts


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", CASES)
def test_old_list_is_leaving_plus_kept(name):
    m = tc.model(name)
    vol, old = m["volume"], m["surface"]
    dims = vol.dims
    worst = 0.0
    for s in shifts(dims):
        lv = sm.leaving(vol, s, surface=old)
        new = sm.shifted(vol, s).extract(1)
        kept = lv["kept"]
        # the shifted volume lists exactly the kept crossings, in the same order
        assert np.array_equal(sm.map_back(new["voxel"], s, dims), old["voxel"][kept]), s
        assert np.array_equal(new["axis"], old["axis"][kept])
        # disjoint by construction (a mask and its complement); together they are the old list
        assert lv["points"].shape[1] + new["points"].shape[1] == old["points"].shape[1]
        assert np.array_equal(lv["voxel"], old["voxel"][~kept]) and np.array_equal(lv["axis"], old["axis"][~kept])
        assert same_bits(new["normals"], old["normals"][:, kept]) and same_bits(new["intensity"], old["intensity"][kept])
        if new["points"].shape[1]:
            d = float(np.abs(new["points"].astype(np.float64) - old["points"][:, kept].astype(np.float64)).max())
            worst = max(worst, d)
            assert d <= 1e-5, (s, d)
        assert 0 <= lv["n_no_normal"] <= old["n_no_normal"]
        if s == (0, 0, 0):
            assert kept.all() and lv["n_no_normal"] == 0
        if abs(s[0]) >= dims[0] or abs(s[1]) >= dims[1]:
            assert not kept.any() and new["points"].shape[1] == 0 and lv["n_no_normal"] == old["n_no_normal"]
            assert not sm.shifted(vol, s).weight.any()
    print(f"{name}: kept points move by at most {worst:.3g} m")
    if name == "room_color":
        assert np.ptp(old["intensity"]) > 0.1


def test_room_leaving_counts():
    m = tc.model("room")
    vol, old = m["volume"], m["surface"]
    assert old["points"].shape[1] == 3410
    got = [sm.leaving(vol, s, surface=old)["points"].shape[1] for s in ((3, -2, 1), (-1, 0, 0), (1, 0, 0), (4, 4, 4))]
    assert got == [612, 52, 0, 894]
    # the narrower predicate "V or N leaves" would lose crossings for good: they would be neither streamed nor kept
    s = (-1, 0, 0)
    narrow = ~sm.ends_stay_mask(old["voxel"], old["axis"], s, vol.dims)
    assert int(narrow.sum()) < 52


def test_planes_move_and_fresh_slab():
    vol = tc.model("odd")["volume"]
    dx, dy, dz = vol.dims
    sh = sm.shifted(vol, (2, 0, 1))
    assert same_bits(sh.tsdf[:dz - 1, :, :dx - 2], vol.tsdf[1:, :, 2:]) and not sh.weight[dz - 1:].any() and not sh.weight[:, :, dx - 2:].any()
    back = sm.shifted(sh, (-2, 0, -1))
    # the slab that left is fresh, not restored; the rest is where it was
    assert same_bits(back.tsdf[1:, :, 2:], vol.tsdf[1:, :, 2:]) and not back.weight[0].any() and not back.weight[:, :, :2].any()
    assert (vol.weight[0].any() or vol.weight[:, :, :2].any()) and same_bits(back.origin, vol.origin) and not back.total.any()


def test_origin_returns_bit_for_bit():
    for name in CASES:
        vol = tc.model(name)["volume"]
        v = vol
        seen = []
        for s in ((1, 0, 0), (1, 0, 0), (1, 0, 0), (-3, 0, 0)):
            v = sm.shifted(v, s)
            seen.append(v.origin.copy())
        assert same_bits(v.origin, vol.origin) and not v.total.any()
        assert same_bits(seen[2], sm.origin_after(vol.origin, (3, 0, 0), vol.voxel)) and seen[2][0] > vol.origin[0]
    o = np.float32(-2.4)
    assert sm.origin_after([o, o, o], (3, 0, 0), 0.11)[0] == np.float32(np.float64(o) + 3.0 * np.float64(np.float32(0.11)))


class _StubContext:
    """what TsdfVolume's constructor needs of a context"""

    def tsdf_create(self, **kw):
        p = binding.TsdfParams()
        p.voxel = kw["voxel"]
        return p


def following_volume(voxel):
    """a TsdfVolume whose shift() is recorded and not made: (vol, shifts, min_weights)"""
    vol = TsdfVolume(_StubContext(), dims=(8, 8, 8), voxel=voxel, origin=(0, 0, 0), trunc=0.25)
    shifts, min_weights = [], []

    def shift(s, min_weight=None):
        shifts.append(tuple(int(x) for x in s))
        min_weights.append(min_weight)
        vol.total = vol.total + np.asarray(s, np.int64)
        return dict(points=np.zeros((3, 0), np.float32))

    vol.shift = shift
    return vol, shifts, min_weights


def pose_at(c):
    P = np.eye(4)
    P[:3, 3] = c
    return P


def test_follow_rounding():
    voxel = 0.0625  # (dyadic: the products below are exact)
    vol, shifts, min_weights = following_volume(voxel)
    vol.follow_min_weight = 3
    assert vol.follow(pose_at((1.0, 2.0, 3.0)), every=2) is None and np.array_equal(vol.follow_ref, (1.0, 2.0, 3.0))
    # half a voxel backwards rounds away from zero: k = -1, below `every` = 2 -- nothing moves
    assert np.array_equal(TsdfVolume.follow_steps((1.0 - 0.5 * voxel, 2.0, 3.0), vol.follow_ref, voxel), (-1, 0, 0))
    assert vol.follow(pose_at((1.0 - 0.5 * voxel, 2.0, 3.0)), every=2) is None and shifts == []
    # ... and with every = 1 it does, by one voxel, and the reference advances by exactly that
    assert vol.follow(pose_at((1.0 - 0.5 * voxel, 2.0, 3.0)), every=1) is not None
    assert shifts == [(-1, 0, 0)] and min_weights == [3]
    assert np.array_equal(vol.follow_ref, (1.0 - voxel, 2.0, 3.0)) and np.array_equal(vol.total, (-1, 0, 0))
    # exactly `every` voxels: it shifts (>=), all three axes by what they have moved, small ones included
    ref = vol.follow_ref.copy()
    c = ref + np.array([0.0, 2 * voxel, -0.49 * voxel])
    assert vol.follow(pose_at(c), every=2) is not None and shifts[-1] == (0, 2, 0)
    c = vol.follow_ref + np.array([1.5 * voxel, -3 * voxel, 0.5 * voxel])
    assert vol.follow(pose_at(c), every=3) is not None and shifts[-1] == (2, -3, 1)
    # just below: 1.49 voxels round to 1
    n = len(shifts)
    assert vol.follow(pose_at(vol.follow_ref + np.array([1.49 * voxel, 0, 0])), every=2) is None and len(shifts) == n
    # the independent statement of the rounding agrees on a sweep that includes every half
    for q in np.arange(-3.0, 3.01, 0.25):
        got = TsdfVolume.follow_steps((q * voxel, 0.0, 0.0), (0.0, 0.0, 0.0), voxel)
        assert np.array_equal(got, sm.follow_steps((q * voxel, 0.0, 0.0), (0.0, 0.0, 0.0), voxel)), q
    assert TsdfVolume.follow_steps((2.5 * voxel, -2.5 * voxel, 0.0), (0, 0, 0), voxel).tolist() == [3, -3, 0]
