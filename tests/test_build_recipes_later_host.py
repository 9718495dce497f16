"""The second recipe table of build.py (build.LATER_PROGRAMS: the rows added since tests/test_build_recipes_host.py pinned
build.PROGRAMS and build.DEFAULT) and what build.plan makes of each of its rows.  No compiler is run."""
import os

from icp_slam_prototype_amd import build

PLANS = {name: build.plan(name) for name in list(build.PROGRAMS) + list(build.LATER_PROGRAMS)}
KINDS = {row["kind"] for row in build.PROGRAMS.values()}


def test_the_two_tables_share_no_name_and_one_shape():
    assert build.LATER_PROGRAMS and not set(build.PROGRAMS) & set(build.LATER_PROGRAMS)
    for name, row in build.LATER_PROGRAMS.items():
        assert row["kind"] in KINDS and row["doc"], name
        assert row["kind"] != "sanitized" or name.endswith("_sanitized"), name
    assert {"test_tsdf_esdf", "esdf_host_sanitized"} <= set(build.LATER_PROGRAMS)


def test_every_later_source_exists():
    for name in build.LATER_PROGRAMS:
        p = PLANS[name]
        assert p.sources and all(os.path.isfile(s) for s in p.sources), (name, p.sources)


def test_outputs_and_objects_are_unique_across_both_tables_and_the_library():
    outs = [p.out for p in PLANS.values()]
    assert len(set(outs)) == len(outs) and all(os.path.dirname(o) == build.LIBDIR for o in outs)
    assert build.LIB not in outs
    objs = [os.path.join(build.LIBDIR, s.rsplit(".", 1)[0] + ".o") for s in build.SOURCES]
    for p in PLANS.values():
        objs += [c[c.index("-o") + 1] for c in p.commands if "-c" in c]
    assert all(o.endswith(".o") and os.path.dirname(o) == build.LIBDIR for o in objs)
    assert len(set(objs)) == len(objs), sorted(o for o in set(objs) if objs.count(o) > 1)


def test_the_defaults_keep_the_tables_apart():
    assert not set(build.DEFAULT) & set(build.LATER_PROGRAMS)
    assert build.LATER_DEFAULT == [n for n, row in build.LATER_PROGRAMS.items() if not row["kind"].startswith("sanitized")]
    assert "test_tsdf_esdf" in build.LATER_DEFAULT and "esdf_host_sanitized" not in build.LATER_DEFAULT


def test_a_later_row_is_rebuilt_after_what_it_reads():
    rules = {os.path.join(build.CSRC, h) for h in os.listdir(build.CSRC) if h.endswith(".h")}
    assert os.path.join(build.CSRC, "esdf_rule.h") in rules
    assert rules <= set(PLANS["esdf_host_sanitized"].deps) and build.LIB in PLANS["esdf_host_sanitized"].deps
    assert os.path.join(build.HERE, "include", "icp_tsdf.hpp") in PLANS["test_tsdf_esdf"].deps
