"""The mapped nearest-neighbour lookup's model (tests/map_nn_model.py, icp.cpp:347-486): the literal walk and the
vectorised restatement agree on random maps, and hand-built maps pin each quirk of the reference's walk.  No GPU."""
import numpy as np
import pytest

import map_model as mm
import map_nn_model as nm

V = (150, 150, 150)


def both(model, q, literal=True):
    b = nm.nearest_vectorised(nm.Lookup(model), q)
    if not literal:
        return b
    a = nm.nearest_literal(model, q)
    assert (np.float32(a[0]).view(np.uint32), a[1], a[2]) == (np.float32(b[0]).view(np.uint32), b[1], b[2]), (q, a, b)
    return a


def off(w, dx=0, dy=0, dz=0):
    return (w[0] + dx, w[1] + dy, w[2] + dz)


def near(q, dx=0.0, dy=0.0, dz=0.0):
    return (np.float32(q[0] + dx), np.float32(q[1] + dy), np.float32(q[2] + dz))


def test_constants():
    assert nm.MAX_RADIUS == 44
    assert sum(24 * r * r - 24 * r + 8 for r in range(1, 44)) == 636056


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_literal_and_vectorised_agree_on_random_maps(seed):
    rng = np.random.default_rng(seed)
    m = mm.Map()
    # a dense cloud in a 0.6 m box near (5, 5, 5), a sparse one around it, a few clamped far points
    m.update(mm.ADD_CLOUD, rng.uniform(4.8, 5.4, (3, 600)).astype(np.float32), 180)
    m.update(mm.ADD_CLOUD, rng.uniform(4.0, 6.0, (3, 40)).astype(np.float32), 180)
    m.update(mm.ADD_ASSOCIATED, np.repeat(rng.uniform(4.5, 5.5, (3, 50)).astype(np.float32), 2, axis=1), 255)
    q = np.concatenate([rng.uniform(4.7, 5.5, (3, 12)), rng.uniform(4.2, 5.8, (3, 3))], axis=1).astype(np.float32)
    for i in range(q.shape[1]):
        both(m, q[:, i])


def test_centre_returns_at_once():
    # the centre voxel holds a point 0.5 m away (y clamped to voxel 0); a point 0.03 m away lies in shell 1
    q = (np.float32(5.01), np.float32(-0.01), np.float32(5.01))
    v = mm.voxel(q)
    a = (np.float32(5.01), np.float32(-0.51), np.float32(5.01))
    b = (np.float32(5.04), np.float32(-0.01), np.float32(5.01))
    assert mm.voxel(a) == v and mm.voxel(b) == off(v, 1)
    m = mm.Map()
    m.update(mm.ADD_CLOUD, np.array([a, b], np.float32).T, 180)
    d, lst, idx = both(m, q)
    assert (lst, idx) == (mm.KEYPOINTS, 0) and d == nm.pair_dist(q, a)
    m2 = mm.Map()
    m2.update(mm.ADD_CLOUD, np.array([b], np.float32).T, 180)
    assert both(m2, q)[1:] == (mm.KEYPOINTS, 0)


def test_plus_faces_are_not_walked():
    # half-open ranges: (vx + r, vy + r, vz) is read in no shell; its mirror (vx - r, vy - r, vz) is
    q = nm.voxel_centre(V)
    for r in (1, 2, 5):
        for w, found in ((off(V, r, r), False), (off(V, -r, -r), True), (off(V, r - 1, r), False),
                         (off(V, -r + 1, r), r > 1), (off(V, 0, 0, r), r > 1), (off(V, r - 1, r - 1, r), False)):
            m = mm.Map()
            nm.plant(m, [(w, near(q, 0.1))])
            d, lst, idx = both(m, q, literal=found or r == 1)
            assert (lst == mm.POINTS) == found, (r, w)


def test_out_of_range_plane_skips_its_twin():
    # vx - r < 0 skips block 1 at radius r, so the in-range plane x = vx + r is not read either
    for vx, found in ((2, False), (3, True)):
        v = (vx, 150, 150)
        q = nm.voxel_centre(v)
        m = mm.Map()
        nm.plant(m, [(off(v, 3), near(q, 0.3))])
        assert (both(m, q, literal=found)[1] == mm.POINTS) == found
    # block 2 needs both y planes, block 3 both z planes
    for v, w, found in (((150, 1, 150), (150, 3, 150), False), ((150, 2, 150), (150, 4, 150), True),
                        ((150, 150, 298), (150, 150, 296), False), ((150, 150, 297), (150, 150, 295), True)):
        q = nm.voxel_centre(v)
        m = mm.Map()
        nm.plant(m, [(w, near(q, 0.3))])
        assert (both(m, q, literal=found)[1] == mm.POINTS) == found, v


def test_block1_z_overrun_reads_the_flat_neighbour():
    # from (150, 150, 2), shell 3 reads (147, y, -1) at flat offset ((147 * 300 + y) * 300 - 1) = voxel (147, y - 1, 299)
    v = (150, 150, 2)
    q = nm.voxel_centre(v)
    w = (147, 149, 299)
    assert nm.visits(v, w) == [(3, 2 * ((150 - 147) * 6 + (-1 - (-1))) + 0)]
    m = mm.Map()
    nm.plant(m, [(w, near(q, 0.25))])
    d, lst, idx = both(m, q)
    assert (lst, idx) == (mm.POINTS, 0) and d == nm.pair_dist(q, near(q, 0.25))
    # and upwards: from (150, 150, 297), shell 4 reads (154, y, 300) = voxel (154, y + 1, 0)
    v = (150, 150, 297)
    q = nm.voxel_centre(v)
    m = mm.Map()
    nm.plant(m, [((154, 149, 0), near(q, 0, 0.25))])
    assert both(m, q)[1] == mm.POINTS


def test_table_ends_are_skipped():
    # x = y = 0, z < 0: outside the table (unpinned), read as nothing
    v = (3, 0, 1)
    q = nm.voxel_centre(v)
    assert all(s == 0 for s, _ in nm.visits(v, v))
    m = mm.Map()
    assert both(m, q)[1] == nm.EMPTY  # (the query is within 0.75 m of the origin: the zero point wins at the centre)


def test_visit_order_ties():
    q = nm.voxel_centre(V)
    # same shell, same (y, z) step: the x - r plane is read before x + r
    a, b = near(q, -0.25), near(q, 0.25)
    assert nm.pair_dist(q, a) == nm.pair_dist(q, b)
    m = mm.Map()
    nm.plant(m, [(off(V, 2), b), (off(V, -2), a)])
    assert both(m, q)[1:] == (mm.POINTS, 1)
    # same shell, different blocks: block 1 before block 3
    m = mm.Map()
    nm.plant(m, [(off(V, 0, 0, -2), a), (off(V, 2, 1, 1), b)])
    assert both(m, q)[1:] == (mm.POINTS, 1)
    # earlier shell keeps the tie against a later one
    m = mm.Map()
    nm.plant(m, [(off(V, 3), a), (off(V, 0, -2), b)])
    assert both(m, q)[1:] == (mm.POINTS, 1)


def test_zero_point_wins_near_the_origin():
    q = (np.float32(0.1), np.float32(0.2), np.float32(0.15))
    m = mm.Map()
    d, lst, idx = both(m, q)
    assert (lst, idx) == (nm.EMPTY, -1) and d == nm.pair_dist(q, nm.ZERO)
    # a filled centre farther than the origin: shell 1's first empty voxel gives |q| and the walk goes on (>= 0.2)
    v = mm.voxel(q)
    m = mm.Map()
    nm.plant(m, [(v, near(q, 0.76))])
    d, lst, idx = both(m, q)
    assert lst == nm.EMPTY and d == nm.pair_dist(q, nm.ZERO)
    # a closer stored point farther out still beats it
    m = mm.Map()
    nm.plant(m, [(v, near(q, 0.76)), (off(v, -2, 1, 1), near(q, 0.1))])
    assert both(m, q)[1:] == (mm.POINTS, 1)


def test_radius_43_is_the_last_shell():
    q = nm.voxel_centre(V)
    for r, found in ((43, True), (44, False)):
        m = mm.Map()
        nm.plant(m, [(off(V, -r), near(q, 0.3))])
        assert (nm.nearest_vectorised(nm.Lookup(m), q)[1] == mm.POINTS) == found
    m = mm.Map()
    nm.plant(m, [(off(V, -43), near(q, 0.3))])
    assert nm.nearest_literal(m, q)[1] == mm.POINTS


def test_walk_goes_on_past_a_hit_above_the_stop_value():
    q = nm.voxel_centre(V)
    m = mm.Map()
    nm.plant(m, [(off(V, -1), near(q, 0.3)), (off(V, 5, 2, 1), near(q, 0, 0.1))])
    d, lst, idx = both(m, q)
    assert (lst, idx) == (mm.POINTS, 1) and d == nm.pair_dist(q, near(q, 0, 0.1))
    # below 0.2 the walk stops after its shell
    m = mm.Map()
    nm.plant(m, [(off(V, -1), near(q, 0.15)), (off(V, 5, 2, 1), near(q, 0, 0.1))])
    assert both(m, q)[1:] == (mm.POINTS, 0)


def test_non_finite_queries_find_nothing():
    m = mm.Map()
    m.update(mm.ADD_CLOUD, np.array([[5.0, 5.0, 5.0], [np.nan, 1.0, 1.0]], np.float32).T, 180)
    lk = nm.Lookup(m)
    for q in ((np.nan, 5.0, 5.0), (np.inf, 5.0, 5.0), (5.0, -np.inf, 5.0)):
        assert nm.nearest_vectorised(lk, q) == (nm.MAX_DIST, nm.NONE, -1)
    assert nm.nearest_literal(m, (np.nan, 5.0, 5.0)) == (nm.MAX_DIST, nm.NONE, -1)
