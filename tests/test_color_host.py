"""Colored ICP on the host (include/icpk.h, K17): the numpy model of tests/color_model.py against the properties the
rule is built for -- no GPU, no library."""
import numpy as np
import pytest

import color_model as cm
from icp_slam_prototype_amd import synth


def _cloud(n, seed):
    """a jittered patch with normals near +z, some of them tilted, and a random intensity"""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(0, 0.3, n), rng.uniform(0, 0.3, n), 1 + rng.normal(0, 0.003, n)]).astype(np.float32)
    nrm = np.stack([rng.normal(0, 0.05, n), rng.normal(0, 0.05, n), np.ones(n)])
    nrm = (nrm / np.linalg.norm(nrm, axis=0)).astype(np.float32)
    return pts, nrm, rng.uniform(0, 1, n).astype(np.float32)


def test_sums_do_not_depend_on_the_order_of_the_cloud():
    pts, nrm, inten = _cloud(700, 1)
    S = cm.gradient_sums(pts, nrm, inten, 0.04)
    perm = np.random.default_rng(2).permutation(700)
    Sp = cm.gradient_sums(pts[:, perm], nrm[:, perm], inten[perm], 0.04)
    assert np.array_equal(Sp, S[perm]) and S[:, 0].min() >= 1 and (S[:, 7:] != 0).any()
    g = cm.gradients_from_sums(S, nrm, 0.04, 4)
    gp = cm.gradients_from_sums(Sp, nrm[:, perm], 0.04, 4)
    assert g.tobytes() == np.ascontiguousarray(gp[:, np.argsort(perm)]).tobytes() and (g != 0).any()


def test_constant_intensity_has_no_gradient():
    pts, nrm, _ = _cloud(500, 3)
    g, S = cm.gradients(pts, nrm, np.full(500, 0.37, np.float32), 0.04)
    assert not S[:, 7:].any() and S[:, 1].any()
    assert not g.any()


def test_linear_field_on_a_plane():
    """I = a x + b y + c on the exact plane z = 1 with jittered points: the gradient is (a, b, 0).

    The bound.  Per neighbour the fit sees u / r rounded to 2^-15 (half a step: 2^-16) and the intensity difference
    rounded likewise; the intensities themselves are floats in [0, 1] (2^-25 each, negligible).  With unquantised offsets
    the least-squares solution of an exactly linear field is exact; quantisation perturbs every equation q . g' = c by at
    most |g'| 2^-16 sqrt(2) + 2^-16 in units of the intensity range, where g' = r (a, b) is the gradient per radius.  A
    least-squares solution moves by at most the perturbation's norm over the smallest singular value of the offsets:
    with neighbours filling the disc, sum q q^T / m has both in-plane eigenvalues about 1/4 (of F^2), so the error of g'
    is at most about 2 (|g'| sqrt(2) + 1) 2^-16, and of the gradient that over r:
        |error| <= 2^-15 (1 + sqrt(2) r |(a, b)|) / r
    -- "2^-15 of the intensity range over the radius", times a factor near 1.  The float narrowing of the result adds
    2^-24 relative."""
    rng = np.random.default_rng(4)
    r = 0.04
    v, u = np.mgrid[0:40, 0:40]
    pts = np.stack([u.ravel() * 0.01 + rng.uniform(-0.003, 0.003, 1600), v.ravel() * 0.01 + rng.uniform(-0.003, 0.003, 1600),
                    np.ones(1600)]).astype(np.float32)
    nrm = np.tile(np.float32([[0], [0], [1]]), (1, 1600))
    a, b, c = 1.1, -0.7, 0.45
    inten = (a * pts[0].astype(np.float64) + b * pts[1].astype(np.float64) + c).astype(np.float32)
    assert inten.min() >= 0 and inten.max() <= 1
    g, S = cm.gradients(pts, nrm, inten, r, 6)
    bound = 2.0 ** -15 * (1 + np.sqrt(2) * r * np.hypot(a, b)) / r
    err = np.abs(g.astype(np.float64) - np.array([[a], [b], [0.0]]))
    inner = (S[:, 0] >= 30)  # the disc is full away from the rim of the patch
    print("linear field: worst error", err[:, inner].max(), "bound", bound, "points", int(inner.sum()))
    assert inner.sum() > 900 and err[:, inner].max() <= bound
    assert (g[2] == 0).all() or np.abs(g[2]).max() <= bound


def test_lambda_one_is_point_to_plane(oracle):
    rng = np.random.default_rng(5)
    tgt, tn, tc = _cloud(2000, 6)
    tn[:, rng.random(2000) < 0.1] = 0
    src = (tgt[:, rng.integers(0, 2000, 1500)] + rng.normal(0, 0.004, (3, 1500))).astype(np.float32)
    sc = rng.uniform(0, 1, 1500).astype(np.float32)
    g, _ = cm.gradients(tgt, tn, tc, 0.04)
    idx, dist = oracle.nn_bruteforce(src, tgt, threads=oracle.max_threads())
    want, wcnt = cm.sums_p2l(src, tgt, tn, idx, dist, 0.01)
    got, cnt = cm.sums(src, tgt, tn, g, tc, sc, idx, dist, 0.01, 1.0)
    assert cnt == wcnt and 0 < cnt < 1500
    assert np.array_equal(got, want)
    # (cm.sums_p2l stands beside cm.sums in one file; the independent reference is the oracle's C restatement of K5)
    osums, ocnt = oracle.sums_p2l_canonical(src, tgt, tn, idx, dist, 0.01)
    assert cnt == ocnt and np.array_equal(got.view(np.uint64), np.asarray(osums, np.float64).view(np.uint64))
    other, _ = cm.sums(src, tgt, tn, g, tc, sc, idx, dist, 0.01, 0.5)
    assert not np.array_equal(other[:27], want[:27]) and other[27] == want[27]


def test_flat_wall_end_to_end(oracle):
    """The wall of the issue (synth.textured_wall_pair, relief 0): point-to-plane has nothing to hold the in-plane motion
    with and is degenerate at the first step; the joint step recovers the pose.  The bound asserted is twice what this
    model measured (color_model.WALL_MEASURED, recorded in DESIGN.md K17)."""
    p = cm.wall_pair()
    tn = p["target_normals"]
    g, S = cm.gradients(p["target"], tn, p["target_intensity"], cm.WALL_RADIUS, cm.WALL_MIN_NB)
    assert (g != 0).any(0).mean() > 0.99
    plain = cm.align(p["source"], p["target"], tn, g, p["target_intensity"], p["source_intensity"], oracle,
                     iterations=cm.WALL_ITER, colored=False)
    assert plain["status"] == 2 and plain["iterations"] == 0
    m = cm.align(p["source"], p["target"], tn, g, p["target_intensity"], p["source_intensity"], oracle,
                 iterations=cm.WALL_ITER, lambda_geometric=cm.LAMBDA)
    er, et = cm.pose_errors(m["T"], p["T_true"])
    print("flat wall, lambda_geometric 0.968: rotation", er, "translation", et)
    assert m["status"] == 0 and m["iterations"] == cm.WALL_ITER
    assert er <= 2 * cm.WALL_MEASURED[0] and et <= 2 * cm.WALL_MEASURED[1]


def test_textured_wall_pair_shapes():
    p = synth.textured_wall_pair(rows=6, cols=8, relief=0.003, seed=2)
    assert p["source"].shape == p["target"].shape == (3, 48) and p["source"].dtype == np.float32
    for k in ("source_intensity", "target_intensity"):
        assert p[k].shape == (48,) and p[k].dtype == np.float32 and p[k].min() >= 0.05 - 1e-6 and p[k].max() <= 0.95 + 1e-6
    moved = p["T_true"][:3, :3] @ p["source"].astype(np.float64) + p["T_true"][:3, 3:4]
    assert np.abs(moved[2] - 2.0).max() <= 0.003 + 1e-6 and np.ptp(p["target"][2]) > 0
    assert np.array_equal(synth.textured_wall_pair(rows=6, cols=8, relief=0.003, seed=2)["source"], p["source"])
