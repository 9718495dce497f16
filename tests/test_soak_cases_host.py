"""The case generators of the newer soak slices (tests/soak_cases.py: flavour_cases, neighbourhood_cases) without a GPU
and without the library: the cases of tests/test_gpu_soak.py's slices are the same on every pass, hold the geometry and
the settings they are there for, and are cases the numpy models take to the end."""
import numpy as np
import pytest

import normals_model as nm
import soak_cases as sc


def _cases(name):
    n, seed0 = sc.SLICES[name]
    gen = sc.neighbourhood_cases if name in sc.FEATURES else sc.flavour_cases
    return list(gen(name, n, seed0))


@pytest.mark.parametrize("name", sc.FEATURES + sc.FLAVOURS)
def test_two_passes_give_the_same_bytes(name):
    a, b = _cases(name), _cases(name)
    assert len(a) == len(b) == sc.SLICES[name][0]
    assert [sc.case_bytes(x) for x in a] == [sc.case_bytes(x) for x in b]
    assert len({x["name"] for x in a}) == len(a)  # (a log line names one case)


@pytest.mark.parametrize("feature", sc.FEATURES)
def test_neighbourhood_slice_holds_its_geometry_and_its_model_takes_every_case(feature):
    cases = _cases(feature)
    assert {c["kind"] for c in cases} == set(sc.ALL_KINDS) and len(sc.ALL_KINDS) == len(sc.KINDS) + 2 == 9
    assert {c["rclass"] for c in cases} == set(sc.RADIUS_CLASSES)
    two_sided = feature != "color_gradients"  # (its sums exist for the target alone)
    assert set(sc.FEATURE_SIDES[feature]) == ({0, 1} if two_sided else {1})
    ties = 0
    for c in cases:
        pts, r = c["pts"], np.float32(c["r"])
        assert pts.dtype == np.float32 and pts.shape[0] == 3 and 1 <= pts.shape[1] <= 4000
        assert np.isfinite(r) and r > 0 and float(r) == c["r"]
        u = sc.distinct_finite(pts)
        assert u.shape[1] == c["distinct"]
        if c["rclass"] == "above":
            assert pts.shape[1] <= sc.WHOLE_CLOUD_MAX_POINTS
        if u.shape[1] >= 2:
            i, j = nm.neighbour_pairs(pts, r)
            d = nm.pair_dist(pts[:, i], pts[:, j])
            fin = int(np.isfinite(pts).all(0).sum())
            if c["rclass"] == "below":    # below every spacing: only a point itself and its duplicates are within reach
                assert not (d > 0).any()
            elif c["rclass"] == "above":  # above the diameter: every finite point has every other
                assert i.size == fin * fin
            elif c["rclass"] == "tie":    # a lattice distance as float32: pairs at exactly d == r
                assert c["kind"] in sc.LATTICE_KINDS and np.count_nonzero(d == r) >= 100
                ties += 1
            else:                         # a drawn radius: neighbourhoods a model call gets through quickly
                assert np.count_nonzero(d > 0) <= 1.5 * sc.MEAN_NEIGHBOURS * fin
        sc.run_neighbourhood_model(c)  # (to the end, its own asserts holding)
    assert ties >= 1
    assert any(c["distinct"] == 1 and c["pts"].shape[1] > 1 for c in cases)  # one repeated point
    assert any(c["kind"] == "plane_x" and np.ptp(sc.distinct_finite(c["pts"])[0]) == 0 for c in cases)  # nx = 1
    assert any(c["kind"] == "line_z" and not np.ptp(sc.distinct_finite(c["pts"])[:2], axis=1).any() for c in cases)
    assert any(not np.isfinite(c["pts"]).all() for c in cases)
    assert any(c["distinct"] < np.isfinite(c["pts"]).all(0).sum() for c in cases)  # exact duplicates
    if feature in ("score", "fpfh"):
        assert any(c["zero_noise"] for c in cases)
        zero = next(c for c in cases if c["zero_noise"])
        assert (zero["source"][:, :, None] == zero["pts"][:, None, :]).all(0).any(1).sum() >= 0.5 * zero["source"].shape[1]
    if feature == "score":
        assert all(np.array_equal(c["poses"][0], np.eye(4, dtype=np.float32)) for c in cases)
        assert all(not np.isfinite(c["poses"]).all() for c in cases)


@pytest.mark.parametrize("flavour", sc.FLAVOURS)
def test_flavour_slice_holds_its_settings(flavour):
    cases = _cases(flavour)
    reads_normals = flavour != "robust_kabsch"
    for c in cases:
        s, t, kw = c["source"], c["target"], c["settings"]
        assert s.dtype == t.dtype == np.float32 and 50 <= s.shape[1] <= 20000 and 50 <= t.shape[1] <= 20000
        assert 1 <= kw["max_iterations"] <= 12 and kw["min_pairs"] >= 3
        assert kw["fixed_iterations"] == 1 or 1e-6 <= kw["threshold"] <= 1e-3
        assert ("target_normals" in c) == reads_normals and ("source_normals" in c) == (flavour == "plane_to_plane")
        assert ("robust" in c) == flavour.startswith("robust")
    kinds = {c["kind"] for c in cases}
    assert "kinect" in kinds and len(kinds & set(sc.ALL_KINDS)) >= 5
    assert {c["settings"]["fixed_iterations"] for c in cases} == {0, 1}
    assert any(c["settings"]["min_pairs"] > c["source"].shape[1] for c in cases)
    assert any(3 < c["settings"]["min_pairs"] <= c["source"].shape[1] for c in cases)
    zero = [c for c in cases if c["zero_noise"]]
    assert zero and all((c["source"][:, :64, None] == c["target"][:, None, :]).all(0).any(1).all() for c in zero)
    if reads_normals:
        assert {c["normals"] for c in cases} == {"estimated", "uploaded"}
        assert any(c["zero_normals"] for c in cases)
    if flavour.startswith("robust"):
        assert {c["robust"]["kernel"] for c in cases} == {0, 1, 2} and {c["robust"]["scale_mode"] for c in cases} == {0, 1}
        assert {c["robust"]["trim"] for c in cases} == {1.0, 0.8, 0.5, 1e-6}
    if flavour == "plane_to_plane":
        assert {c["epsilon"] for c in cases} == {1e-3, 1e-2, 1.0}
    if flavour == "colored":
        assert {c["lambda_geometric"] for c in cases} == {0.0, 0.5, 0.968, 1.0}
