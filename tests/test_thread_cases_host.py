"""The thread scripts on the host (tests/thread_cases.py): the completeness table against binding.Context and the six
functions over a context, the exempt set written out, the scripts the table names, and the dry run.  No GPU and no
library call: tests/test_gpu_threads.py holds at run time that the serial runs do make every non-exempt call."""
import inspect
import re

import history_cases as hc
import test_history_host as hh
import thread_cases as tc
from icp_slam_prototype_amd import binding, sequence

# the names that may be exempt, written out, each with the reason its entry must give
NO_STATE = "holds no device state of the context"
RCCL = "two communicators in one process are outside the threading claim"
EXEMPT = {**{k: NO_STATE for k in hh.EXEMPT},  # stream, source_size, target_size, pair_distance, set_log_callback, close
          "comm_init": RCCL, "comm_destroy": RCCL, "comm_rank": RCCL, "comm_world": RCCL, "comm_broadcast_target": RCCL,
          "comm_gather_results": RCCL, "comm_allreduce_sums": RCCL, "comm_barrier": RCCL,
          "align_query_sharded": RCCL}  # (needs a communicator: history_cases.early_one_rank_communicator is its only user)
# (nothing is exempt for being reachable through an early path of history_cases.EARLY only: transform_target,
# map_release, tsdf_reset and tsdf_release are called by map_tracking and tsdf_follow)


def test_table_covers_the_class_and_the_six_functions_exactly():
    names = hh.public_names() | set(tc.MODULE_FUNCTIONS)
    assert len(names) > 100 + 6 and len(tc.MODULE_FUNCTIONS) == 6
    missing, stale = names - set(tc.COVERAGE), set(tc.COVERAGE) - names
    assert not missing, f"public names without a place in thread_cases.COVERAGE: {sorted(missing)}"
    assert not stale, f"COVERAGE names that binding.Context no longer has: {sorted(stale)}"
    for name, fn in tc.MODULE_FUNCTIONS.items():  # the six are functions whose first argument is the context
        assert fn.__name__ == name and not hasattr(binding.Context, name)
        assert list(inspect.signature(fn).parameters)[0] == "ctx", name


def test_exempt_set_is_the_written_one():
    exempt = {k: str(v) for k, v in tc.COVERAGE.items() if isinstance(v, hc.Exempt)}
    assert set(exempt) == set(EXEMPT)
    for k, reason in EXEMPT.items():
        assert reason in exempt[k], (k, exempt[k])
    assert set(tc.RCCL_NAMES) == {k for k, r in EXEMPT.items() if r == RCCL}
    assert "tests/test_gpu_comm.py" in tc._RCCL


def script_text(name):
    """the text of a hand-written script with that of the helpers of thread_cases it names (one level: they call no
    further ones), and with MultiSequenceRunner's where the script drives one"""
    text = inspect.getsource(tc.BY_NAME[name].fn)
    for helper in sorted(set(re.findall(r"\b(_[a-z_]+)\(", text))):
        fn = getattr(tc, helper, None)
        if inspect.isfunction(fn) and fn.__module__ == tc.__name__:
            text += inspect.getsource(fn)
    if "MultiSequenceRunner" in text:
        text += inspect.getsource(sequence.MultiSequenceRunner)
    return text


def test_every_entry_names_scripts_that_exist_and_call_it():
    for name, users in tc.COVERAGE.items():
        if isinstance(users, hc.Exempt):
            continue
        assert users and set(users) <= set(tc.BY_NAME), (name, users)
        # a probe script is listed because history_cases.COVERAGE lists its probe (tests/test_history_host.py reads the
        # probe's text for the call); nothing else may claim a probe
        probes = {u[len("probe_"):] for u in users if u.startswith("probe_")}
        assert probes == set(hc.COVERAGE.get(name, ())) & set(tc.PROBE_SCRIPTS), name
        for u in set(users) - {"probe_" + p for p in probes}:
            # the method call `.name(`, or the function named to the Log: ctx.call("name", ...)
            assert re.search(r'\.%s\b(?!_)|call\("%s"' % (re.escape(name), re.escape(name)), script_text(u)), \
                f"{u} is listed for {name} and does not call it"
    # the check can fail
    assert not re.search(r"\.tsdf_shift\b(?!_)|call\(\"tsdf_shift\"", script_text("bilateral"))
    assert set(tc.HAND_WRITTEN) <= set(tc.COVERAGE)
    for name, users in tc.HAND_WRITTEN.items():
        assert not any(u.startswith("probe_") for u in users), name


def test_scripts_are_the_old_ones_the_probes_and_the_four():
    names = [s.name for s in tc.SCRIPTS]
    assert len(names) == len(set(names)) == 11 + 21 + 4 == 36
    assert names[11:32] == ["probe_" + k for k in hc.PROBE_ORDER if k != "batch"]
    assert names[32:] == ["bilateral", "tsdf_follow", "model_tracker", "deferred_source"]
    assert set(tc.PROBE_SCRIPTS) == set(hc.PROBES) - {"batch"} and len(hc.PROBES) == 22
    assert all(inspect.isgeneratorfunction(s.fn) for s in tc.SCRIPTS)  # (each can be advanced call by call)


def test_dry_run_builds_every_input_without_the_library(capsys):
    tc.dry_run()
    text = capsys.readouterr().out
    line = [ln for ln in text.splitlines() if ln.startswith("scripts (")]
    assert len(line) == 1 and line[0].startswith("scripts (36): ")
    assert line[0].split(": ", 1)[1].split(", ") == [s.name for s in tc.SCRIPTS]
    for key in ("scenes", "bilateral", "tsdf_follow", "tracker", "deferred", "pair", "frames"):
        assert re.search(r"^%s\s" % key, text, re.M), key
    # two builds, same bytes (the scenes and cases below it are built once per process and read-only:
    # tests/test_history_host.py::test_scene_builders_are_deterministic holds those)
    a, b = tc.build_inputs(), tc.build_inputs()
    assert a is not b and a.keys() == b.keys() and tc.digest(a) == tc.digest(b) == tc.digest(tc.inputs())
    assert a["pair"][0] is not b["pair"][0]
    changed = dict(a, tiny=(a["tiny"][0] + 1, a["tiny"][1]))
    assert tc.digest(changed) != tc.digest(a)  # (the digest does see a changed array)


def test_tracker_frames_move_the_box_once_on_the_models():
    """the sizes of tsdf_follow and model_tracker were settled on the numpy models: what they promise there"""
    import numpy as np

    import tsdf_model
    import tsdf_shift_model as sm

    inp = tc.inputs()
    f = inp["tsdf_follow"]
    vol = tsdf_model.Volume(**f["volume"])
    for d, P in f["frames"][:2]:
        vol.integrate(d, P, f["fx"], f["cx"])
    left = sm.leaving(vol, tc.FOLLOW_SHIFT, 1)
    after = sm.shifted(vol, tc.FOLLOW_SHIFT)
    after.integrate(*f["frames"][2], f["fx"], f["cx"])
    assert len({np.sign(s) for s in tc.FOLLOW_SHIFT}) == 2  # mixed signs
    assert 0 < left["points"].shape[1] < vol.extract(1)["points"].shape[1] and after.extract(1)["points"].shape[1] > 0
    lo, hi = tc.FOLLOW_BOX
    assert all(0 <= a < b <= n for a, b, n in zip(lo, hi, vol.dims))
    # the tracker's frames with their true poses: one shift, by (-1, 0, 0) at frame 1, which streams crossings out; the
    # third frame stays within a quarter of a voxel of the new reference (the tracker's own error is below 0.15 voxel)
    m = inp["tracker"]
    vol, ref, shifts = tsdf_model.Volume(**m["volume"]), None, []
    for k, (d, P) in enumerate(m["frames"]):
        c = P[:3, 3].astype(np.float64)
        ref = c.copy() if ref is None else ref
        q = (c - ref) / np.float64(vol.voxel)
        step = sm.follow_steps(c, ref, np.float64(vol.voxel))
        if (np.abs(step) >= 1).any():
            shifts.append((k, tuple(int(x) for x in step), sm.leaving(vol, step, 1)["points"].shape[1]))
            vol, ref = sm.shifted(vol, step), ref + step * np.float64(vol.voxel)
        else:
            assert np.abs(q).max() < 0.25, (k, q)
        vol.integrate(d, P, m["fx"], m["cx"])
    assert [(k, s) for k, s, _ in shifts] == [(1, (-1, 0, 0))] and shifts[0][2] > 0
