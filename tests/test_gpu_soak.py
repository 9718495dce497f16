"""A bounded, seeded slice of the builder-side soak runs (tools/soak_grid.py, soak_align.py, soak_batch.py) inside
`-m gpu`, so that the driver's own run exercises them: random cloud shapes (lines, lattices, duplicates, tiny / huge
scales), ragged sizes, first (unseeded, expanding) and seeded grid sweeps, whole alignments with threshold exits and
fall-backs, random lock-step groups -- each against an independent path (exact kernel + host loop, or the pairs one by
one), bit for bit.  The seeded chain (sweeps 2 and 3 of a case; icp.cpp:566-593 with the previous match as the bound)
is where a slip in the cube / ball trimming of the grid scan would show.  Each of these four slices is time-boxed (the
cases are the same on every run up to the point where the budget ends).

The slices of the newer flavours (soak_flavours: point-to-plane, robust, plane-to-plane, colored -- grid scan + device
loop against exact kernel + host loop, everything observable bit for bit) and of the neighbourhood kernels
(soak_neighbourhoods: each against the numpy model of its rule, bit for bit) run a fixed number of cases from a fixed
seed (soak_cases.SLICES; tests/test_soak_cases_host.py checks without a GPU what those cases hold) and are not
time-boxed: a slice that cannot finish fails.  A flavour slice must also end at least once in every outcome the
flavour has; the tallies in the docstrings are those of an MI355X."""
import pytest

from icp_slam_prototype_amd import binding

import soak_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from icp_slam_prototype_amd import build

    build.build()
    c = binding.Context(0)
    yield c
    c.close()


def test_soak_slice_grid_sweeps_vs_exact_kernel(ctx):
    done, bad = soak_cases.soak_grid(ctx, 6000, seed0=5000, budget_s=20)
    assert done >= 20 and bad == 0, (done, bad)


def test_soak_slice_grid_sweeps_vs_cpu_oracle(ctx, oracle):
    done, bad = soak_cases.soak_grid(ctx, 60, seed0=7000, budget_s=15, oracle=oracle)
    assert done >= 5 and bad == 0, (done, bad)


def test_soak_slice_alignments_grid_device_loop_vs_exact_host_loop(ctx):
    done, bad = soak_cases.soak_align(ctx, 4000, seed0=9000, budget_s=20)
    assert done >= 20 and bad == 0, (done, bad)


def test_soak_slice_lockstep_batches_vs_single_pairs():
    done, bad = soak_cases.soak_batch(1000, seed0=12000, budget_s=20)
    assert done >= 20 and bad == 0, (done, bad)


def _flavour_slice(ctx, flavour):
    n, seed0 = soak_cases.SLICES[flavour]
    lines = []
    done, bad, tally = soak_cases.soak_flavours(ctx, flavour, n, seed0, log=lines.append)
    print(flavour, done, bad, tally)
    assert done == n and bad == 0, (done, bad, [m for m in lines if m.startswith("MISMATCH")][:5])
    want = [k for k in soak_cases.OUTCOMES if k != "degenerate" or flavour in soak_cases.DEGENERATE_FLAVOURS]
    assert all(tally[k] >= 1 for k in want), tally
    assert sum(tally.values()) == n and tally.get("error", 0) == 0, tally


def test_soak_slice_point_to_plane_alignments(ctx):
    """120 cases: ok_fixed 31, ok_threshold 41, few_at_0 19, few_later 11, degenerate 7 (ok at max_iterations 11)"""
    _flavour_slice(ctx, "p2l")


def test_soak_slice_robust_kabsch_alignments(ctx):
    """120 cases: ok_fixed 36, ok_threshold 22, few_at_0 40, few_later 2 (ok at max_iterations 20); Kabsch solves no
    6 x 6 system"""
    _flavour_slice(ctx, "robust_kabsch")


def test_soak_slice_robust_point_to_plane_alignments(ctx):
    """120 cases: ok_fixed 18, ok_threshold 34, few_at_0 46, few_later 5, degenerate 8 (ok at max_iterations 9)"""
    _flavour_slice(ctx, "robust_p2l")


def test_soak_slice_plane_to_plane_alignments(ctx):
    """120 cases: ok_fixed 50, ok_threshold 22, few_at_0 13, few_later 7, degenerate 2 (ok at max_iterations 26)"""
    _flavour_slice(ctx, "plane_to_plane")


def test_soak_slice_colored_alignments(ctx):
    """120 cases: ok_fixed 31, ok_threshold 36, few_at_0 24, few_later 13, degenerate 4 (ok at max_iterations 12)"""
    _flavour_slice(ctx, "colored")


def _neighbourhood_slice(ctx, feature):
    n, seed0 = soak_cases.SLICES[feature]
    lines = []
    done, bad = soak_cases.soak_neighbourhoods(ctx, feature, n, seed0, log=lines.append)
    assert done == n and bad == 0, (done, bad, [m for m in lines if m.startswith("MISMATCH")][:5])


def test_soak_slice_voxel_downsampling_vs_model(ctx):
    _neighbourhood_slice(ctx, "voxel")


def test_soak_slice_normal_moments_vs_model(ctx):
    _neighbourhood_slice(ctx, "normals")


def test_soak_slice_outlier_filters_vs_model(ctx):
    _neighbourhood_slice(ctx, "filters")


def test_soak_slice_pose_scores_vs_model(ctx):
    _neighbourhood_slice(ctx, "score")


def test_soak_slice_fpfh_and_matches_vs_model(ctx):
    _neighbourhood_slice(ctx, "fpfh")


def test_soak_slice_color_gradient_sums_vs_model(ctx):
    _neighbourhood_slice(ctx, "color_gradients")
