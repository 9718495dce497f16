"""The certainty map's sequential model (tests/map_model.py) on hand-worked sequences, and the library's host voxel
helper icpk_map_voxel (map.cpp:55-85 getVoxelCoordinates) against it.  No GPU needed."""
import numpy as np
import pytest

import map_model as mm
from icp_slam_prototype_amd import binding


def hits_until_filled(rule, d, c0=0):
    m = mm.Map()
    p = (np.float32(5.0), np.float32(5.0), np.float32(5.0))
    if c0:
        m.cert[mm.voxel(p)] = c0
    for k in range(1, 300):
        m.add(rule, p, d)
        if mm.voxel(p) in m.slot:
            return k, m
    return None, m


def test_add_unassociated_fills_on_the_eighth_hit():
    # map.cpp:139-149 with d = 25 from 0: 25, 50, ..., 175 after 7 hits; the 8th sees 175 >= 155
    k, m = hits_until_filled(mm.ADD_UNASSOCIATED, 25)
    assert k == 8
    assert m.certainty(mm.voxel((5, 5, 5))) == 255
    assert len(m.lists[mm.KEYPOINTS]) == 1 and not m.lists[mm.POINTS]


def test_add_associated_fills_on_the_eleventh_hit():
    # map.cpp:104-113 with d = 25: 250 after 10 hits; the 11th sees 250 > 230
    k, m = hits_until_filled(mm.ADD_ASSOCIATED, 25)
    assert k == 11
    assert len(m.lists[mm.POINTS]) == 1 and not m.lists[mm.KEYPOINTS]


def test_add_cloud_fills_on_the_first_hit():
    # map.cpp:249-259 with d = MAX_CONFIDENCE (icp.cpp:62)
    k, m = hits_until_filled(mm.ADD_CLOUD, 180)
    assert k == 1
    assert m.certainty(mm.voxel((5, 5, 5))) == 180
    m.add(mm.ADD_CLOUD, (5, 5, 5), 180)
    assert m.certainty(mm.voxel((5, 5, 5))) == 255  # saturates; the slot stays with the first point
    assert len(m.lists[mm.KEYPOINTS]) == 1


def test_rules_share_one_slot_per_voxel():
    m = mm.Map()
    p, q = (1.01, 2.01, 3.01), (1.02, 2.02, 3.02)  # same voxel
    assert mm.voxel(p) == mm.voxel(q)
    for _ in range(11):
        m.add(mm.ADD_ASSOCIATED, p, 25)
    assert m.slot[mm.voxel(p)] == (mm.POINTS, 0)
    m.add(mm.ADD_UNASSOCIATED, q, 25)  # 255 >= 155, but the slot is taken: nothing appended
    assert not m.lists[mm.KEYPOINTS]
    assert m.is_occupied(q)


def test_cloud_rule_fills_late_when_certainty_was_raised_without_a_fill():
    m = mm.Map()
    p = (2.0, 2.0, 2.0)
    m.cert[mm.voxel(p)] = 100
    m.add(mm.ADD_CLOUD, p, 50)  # 150: not yet
    assert not m.lists[mm.KEYPOINTS]
    m.add(mm.ADD_CLOUD, p, 50)  # 200 >= 180
    assert m.slot[mm.voxel(p)] == (mm.KEYPOINTS, 0)


def test_set_points_keeps_grid_and_slots():
    m = mm.Map()
    m.update(mm.ADD_CLOUD, np.array([[1.0], [1.0], [1.0]], np.float32), 180)
    g, s = dict(m.cert), dict(m.slot)
    m.set_points(np.ones((3, 5), np.float32))
    assert m.cert == g and m.slot == s and len(m.lists[mm.POINTS]) == 5 and len(m.lists[mm.KEYPOINTS]) == 1


def _boundary_values():
    c = mm.C
    vals = [0.0, -0.0, 1e-30, -1e-30, -1.0, -5.0, 1e10, -1e10, np.inf, -np.inf, np.nan, 9.999, 10.0, 10.5, 1e30, -1e30,
            2.0 ** 31 * float(c), 2.0 ** 31 * float(c) * 0.999]
    for k in (1, 2, 3, 7, 10, 100, 150, 299, 300, 301):
        b = np.float32(k) * c
        vals += [float(b), float(np.nextafter(b, np.float32(0))), float(np.nextafter(b, np.float32(np.inf)))]
        vals += [-float(b)]
    return vals


def test_model_voxel_edge_cases():
    assert mm.voxel((np.nan, np.inf, -np.inf)) == (0, 0, 0)
    assert mm.voxel((1e10, -1e10, 2.0 ** 40)) == (0, 0, 0)  # INT_MIN, clamped -- not 299
    assert mm.voxel((-0.0, 9.99, 1e-3)) == (0, 299, 0)
    assert mm.voxel((5.0, 5.0, 5.0)) == (149, 149, 149)  # 5 / float(1/30) = 149.99999


def test_voxel_helper_matches_model():
    vals = _boundary_values()
    rng = np.random.default_rng(1)
    vals += list(rng.uniform(-1, 11, 400).astype(np.float32))
    for i in range(0, len(vals) - 2):
        p = np.array(vals[i:i + 3], np.float32)
        got = tuple(int(v) for v in binding.map_voxel(p))
        assert got == mm.voxel(p), (p, got, mm.voxel(p))


@pytest.mark.parametrize("k", [1, 2, 3, 30, 150, 299, 300])
def test_voxel_helper_at_cell_boundaries(k):
    b = np.float32(k) * mm.C
    for v in (np.nextafter(b, np.float32(0)), b, np.nextafter(b, np.float32(np.inf))):
        p = np.array([v, -v, v], np.float32)
        assert tuple(int(x) for x in binding.map_voxel(p)) == mm.voxel(p)
