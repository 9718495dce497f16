"""The recipe table of build.py (build.PROGRAMS) and what build.plan makes of each row.  No compiler is run."""
import glob
import os

from icp_slam_prototype_amd import build

PLANS = {name: build.plan(name) for name in build.PROGRAMS}
RULES = sorted(glob.glob(os.path.join(build.CSRC, "*.h")))


def test_every_source_a_row_names_exists():
    for name, p in PLANS.items():
        assert p.sources and all(os.path.isfile(s) for s in p.sources), (name, p.sources)


def test_output_paths_are_unique_and_under_lib():
    outs = [p.out for p in PLANS.values()]
    assert len(set(outs)) == len(outs) == len(build.PROGRAMS)
    assert all(os.path.dirname(o) == build.LIBDIR for o in outs)
    assert build.TRACKER_BENCH == PLANS["tracker_bench"].out


def test_no_two_recipes_write_the_same_object_file():
    """(two recipes must never write one .o with different flags; the library's own objects count)"""
    objs = [os.path.join(build.LIBDIR, s.rsplit(".", 1)[0] + ".o") for s in build.SOURCES]
    for p in PLANS.values():
        objs += [c[c.index("-o") + 1] for c in p.commands if "-c" in c]
    assert len(objs) > len(build.SOURCES) and all(o.endswith(".o") and os.path.dirname(o) == build.LIBDIR for o in objs)
    assert len(set(objs)) == len(objs), sorted(o for o in set(objs) if objs.count(o) > 1)


def test_default_is_exactly_the_programs_that_are_not_sanitized():
    """(in the order the entry point built them before there was a table; a new program is appended here too)"""
    assert build.DEFAULT == [
        "test_icp_align", "tracker_bench", "test_map_tracker", "test_map_tracker_fast", "test_map_tracker_dense", "test_voxel",
        "test_normals", "test_filter", "test_gicp", "test_color", "test_score", "test_fpfh", "test_pose_graph", "test_tsdf",
        "test_tsdf_raycast", "test_tsdf_mesh", "test_tsdf_shift", "test_tsdf_refuse", "test_bilateral", "test_pyramid",
        "test_projective", "test_projective_color", "test_fern", "test_frame_odometry", "test_sdf_track", "test_threads",
        "fake_rccl", "solve_probe", "scan_probe"]
    assert set(build.DEFAULT) == {n for n, row in build.PROGRAMS.items() if not row["kind"].startswith("sanitized")}


def test_a_mirror_is_rebuilt_after_any_header_it_can_include():
    mirrors = [n for n, row in build.PROGRAMS.items() if row["kind"] == "mirror"]
    assert mirrors
    for name in mirrors:
        deps = PLANS[name].deps
        for h in ("icp_align.hpp", "icp_map.hpp", "icp_pose_graph.hpp"):
            assert os.path.join(build.HERE, "include", h) in deps, (name, h)
        assert os.path.join(build.ROOT, "include", "icpk.h") in deps and build.LIB in deps, name


def test_whatever_compiles_csrc_is_rebuilt_after_any_csrc_header():
    assert len(RULES) > 10
    n = 0
    for name, p in PLANS.items():
        if any(os.path.dirname(s) == build.CSRC for s in p.sources) or build.PROGRAMS[name]["kind"] in ("sanitized_header", "probe"):
            assert set(RULES) <= set(p.deps), name
            n += 1
    assert n >= 11  # the nine sanitized programs and the two probes, at the least


def test_the_former_builder_names_are_a_frozen_list():
    """(37 names plus build_tracker_bench: one per program there was when the table came; no new row gets one)"""
    assert len(build._FORMER_NAMES) == 37 and "build_tracker_bench" not in build._FORMER_NAMES
    for former, name in build._FORMER_NAMES.items():
        f = getattr(build, former)
        assert name in build.PROGRAMS and f.func is build.program and f.args == (name,), former
    assert not hasattr(build, "build_nothing_test")
