"""INTEGRATION.md's threading row -- one icpk_ctx per thread, no global state -- held to the bit: the scripts of
tests/thread_cases.py (one per public family) run on 8 Python threads at once, each thread on contexts of its own, and
every result must equal, byte for byte, the same script run alone on a fresh context.  ctypes releases the GIL for the
duration of each library call, so the contexts share the GPU's hardware queues and the host's cores for real.

No number here is a tolerance.  The only measured quantities are times: the join time-out (the plan's serial time of
this session x 8 threads x 4, at least 60 s) and the overlap share (per thread, the share of its in-call time during
which another thread was inside a call too; the condition is >= 0.5: runs that serialise give about 0, concurrent ones
close to 1), and both are printed (-s).  The share is taken from wall-clock windows around the calls: it rules out
threads that take turns outside the library (the GIL held, a lock in the binding), not threads that wait for each other
inside a call, and it says nothing about what the device ran side by side.  The work is fixed: 8 threads, 20 repetitions
(5 for the nine neighbourhood probes: NEIGHBOURHOOD_REPEATS says why), 3 ICPK_LOOP_AHEAD settings;
nothing is repeated until it fails and nothing that failed is run again.  After the first thread that raises, the
others finish the call they are in and stop; a thread that outlives the time-out fails the test with the call it was
in, and the rest of the module fails at once without starting GPU work.

The scripts: the 11 hand-written ones, one probe_<name> for each of the 21 probes of tests/history_cases.py but
`batch` (the probe itself on a Traced context: test_adapter_loses_nothing holds that the adapter changes no byte), and
bilateral, tsdf_follow, model_tracker and deferred_source: 36.  The newer families get what the loop step had: the same
script on all threads in lock step, one context repeating the order-sensitive neighbourhood kernels and one walking the
shrink-grow chain of tests/test_gpu_history.py while 7 others load the device, and two contexts that alternate call by
call under a baton (the probe scripts are single calls to test_two_contexts_interleaved_on_one_thread).

Measured on an MI355X with -s (one run of this module; thread wall time, overlap shares min .. max of the 8 threads):
  alone, ms: align_threshold 1.3, align_fallback 0.7, align_fixed_hostloop 1.8, frame_path 3.2, p2l_normals_robust 1.7,
             prepare_chain 2.0, batch 21.6, frames_batch 21.3, map_tracking 5.9, fast 0.4, lifecycle 45.6;
             probe_nn_exact 0.8, _nn_filtered 0.7, _nn_pruned 0.9, _nn_grid 1.2, probe_align_reference 1.5, _kabsch 1.1,
             _point_to_plane 1.2, _plane_to_plane 1.3, _colored 1.8, _robust 1.7, probe_retarget 2.2, probe_normals 0.9,
             probe_voxel 0.8, probe_filter 2.8, probe_color 0.7, probe_score 116.1, probe_fpfh 7.2, probe_tsdf 2.7,
             probe_map 23.8, probe_frontend 3.1, probe_posegraph 23.7; bilateral 1.0, tsdf_follow 2.1,
             model_tracker 4.1, deferred_source 8.7; all 36: 0.32 s (the fixture runs each twice: 1.5 s with the inputs)
  test_concurrent_contexts_equal_serial          3.17 s  0.99 .. 1.00  (288 script runs: 8 x 36)
  test_same_script_on_all_threads                0.68 s  0.99 .. 1.00
  test_two_contexts_interleaved_on_one_thread    0.02 s  (no threads)
  test_threshold_loop_under_load[None / 0 / 3]   2.42 / 3.35 / 2.58 s, 0.98 .. 1.00
  test_adapter_loses_nothing                     0.36 s  (no threads)
  test_same_new_script_on_all_threads            0.53 s  0.99 .. 1.00
  test_neighbourhood_kernels_under_load          2.94 s  1.00 .. 1.00  (thread 0: 0.66 s alone, 0.82 s beside 7 rounds of load)
  test_shrink_grow_chain_under_load              3.27 s  1.00 .. 1.00  (thread 0: 0.69 s alone, 1.22 s beside 7 rounds of
                                                 load; 4.00 s with the chain run alone first)
  test_two_contexts_alternate_call_by_call       0.03 / 0.02 / 0.02 s  (21 + 40, 32 + 24 and 14 + 54 calls; no overlap)
  the module: 23.0 s with tests/test_gpu_threads_cpp.py (0.49 s).  The parent commit's module (7 tests, 11 scripts),
  measured in the same session: 13.6 s without that file; its three tests under load took 3.2 to 3.5 s each there.
  Beside each other a round of load takes 0.4 to 0.5 s against 0.025 s alone; with 33 and 82 rounds (an earlier
  formula) the two new tests under load took 12.7 and 43.8 s and thread 0 was through after 0.43 and 1.42 s.
In that run every byte agreed.
"""
import bisect
import math
import threading
import time
import traceback

import numpy as np
import pytest

import history_cases as hc
import thread_cases as tc
from icp_slam_prototype_amd import binding

pytestmark = pytest.mark.gpu

T = 8                 # threads (fixed: not sized from the machine)
REPEATS = 20          # test_threshold_loop_under_load
MIN_SHARE = 0.5       # overlap condition
ROUNDS = 6            # test_threshold_loop_under_load: rounds of (batch, frame_path) per load thread
_DEAD = []            # a thread outlived its time-out: [what it was in]; no further GPU work in this module


def _alive():
    if _DEAD:
        pytest.fail(f"an earlier test left a thread inside {_DEAD[0]}: no further GPU work in this module")


class _Serial(dict):
    """{script: (first, second, seconds)}; called: the names of all calls the serial runs' Logs saw"""


@pytest.fixture(scope="module")
def serial():
    """Every script twice on fresh contexts, one after the other: {name: (first, second, seconds of the first)}."""
    from icp_slam_prototype_amd import build

    build.build()
    tc.inputs()
    tc.hip()
    out = _Serial()
    out.called = set()
    for s in tc.SCRIPTS:
        runs = []
        for _ in range(2):
            with binding.Context(0) as c:
                tr = tc.Traced(c)
                t0 = time.perf_counter()
                r = s.run(tr)
                runs.append((r, time.perf_counter() - t0))
                out.called |= {name for name, _, _ in tr.log.calls}
        out[s.name] = (runs[0][0], runs[1][0], runs[1][1])  # (the second run's time: the first one pays for first use)
    return out


def _serial_time(serial, names):
    return sum(serial[n][2] for n in names)


# ---- threads --------------------------------------------------------------------------------------------------------
class _Worker:
    """One thread: its Log, what it ran (windows = [(script, t0, t1)]) and what it got (results = [(script, out)])."""

    def __init__(self, k, stop):
        self.k, self.log = k, tc.Log(stop)
        self.windows, self.results, self.error, self.thread = [], [], None, None

    def fresh(self, name):
        """script `name` on a context of its own"""
        c = self.log.call("create", binding.Context, 0)
        try:
            self.on(tc.Traced(c, self.log), name)
        finally:  # (closed even after the stop event: nothing is left open)
            self.log.current = "close"
            self.log.calls.append(("close",) + _timed(c.close))
            self.log.current = None

    def on(self, traced, name):
        t0 = time.perf_counter()
        try:
            self.results.append((name, tc.BY_NAME[name].run(traced)))
        finally:
            self.windows.append((name, t0, time.perf_counter()))


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return t0, time.perf_counter()


def _run_threads(bodies, timeout):
    """bodies[k](worker, barrier): thread k's work.  Started together behind a barrier; joined within `timeout` seconds
    in all.  Returns the workers; fails the test (and the module) if a thread is still alive."""
    stop = threading.Event()
    barrier = threading.Barrier(len(bodies))
    workers = [_Worker(k, stop) for k in range(len(bodies))]

    def main(w, body):
        try:
            barrier.wait(timeout=60)
            body(w, barrier)
        except tc.Stopped:
            pass
        except threading.BrokenBarrierError:
            pass
        except BaseException as e:  # noqa: BLE001 (reported by the test)
            w.error = f"{type(e).__name__}: {e}\n{traceback.format_exc()}"
            stop.set()
            barrier.abort()

    for w, body in zip(workers, bodies):
        w.thread = threading.Thread(target=main, args=(w, body), daemon=True, name=f"icpk-test-{w.k}")
    t0 = time.perf_counter()
    for w in workers:
        w.thread.start()
    for w in workers:
        w.thread.join(max(0.0, timeout - (time.perf_counter() - t0)))
    wall = time.perf_counter() - t0
    hung = [(w.k, w.log.current) for w in workers if w.thread.is_alive()]
    if hung:
        stop.set()
        _DEAD.append(", ".join(f"thread {k}: {call}" for k, call in hung))
        pytest.fail(f"still running after {timeout:.0f} s: {_DEAD[0]}")
    return workers, wall


def _overlap_shares(workers):
    """per thread: the share of its in-call time during which at least one other thread was inside a call too"""
    shares = []
    for w in workers:
        others = sorted((a, b) for v in workers if v is not w for _, a, b in v.log.calls)
        merged = []
        for a, b in others:
            if merged and a <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], b)
            else:
                merged.append([a, b])
        starts = [m[0] for m in merged]
        mine = shared = 0.0
        for _, a, b in w.log.calls:
            mine += b - a
            i = max(bisect.bisect_right(starts, a) - 1, 0)
            while i < len(merged) and merged[i][0] < b:
                shared += max(0.0, min(b, merged[i][1]) - max(a, merged[i][0]))
                i += 1
        shares.append(shared / mine if mine > 0 else 0.0)
    return shares


def _meanwhile(workers, w, t0, t1):
    return {v.k: [n for n, a, b in v.windows if a < t1 and b > t0] for v in workers if v is not w}


def _check(workers, serial, what, wall):
    """no thread raised; every result equals the serial one; the threads did overlap"""
    shares = _overlap_shares(workers)
    print(f"\n{what}: wall {wall:.2f} s, overlap shares " + " ".join(f"{s:.2f}" for s in shares))
    errors = [f"thread {w.k}: {w.error}" for w in workers if w.error]
    assert not errors, "\n".join(errors)
    n = 0
    for w in workers:
        assert len(w.results) == len(w.windows), (w.k, "a script did not finish")
        for (name, got), (_, t0, t1) in zip(w.results, w.windows):
            d = tc.first_difference(got, serial[name][0])
            assert d is None, (f"{what}: thread {w.k}, script {name}: output {d[0]} differs from the serial run at byte {d[1]}; "
                               f"meanwhile the other threads ran {_meanwhile(workers, w, t0, t1)}")
            n += 1
    assert min(shares) >= MIN_SHARE, f"{what}: the threads did not run side by side: overlap shares {shares}"
    return n


# ---- the tests ------------------------------------------------------------------------------------------------------
def test_scripts_alone_are_repeatable(serial, oracle):
    _alive()
    print()
    for name, (a, b, dt) in serial.items():
        print(f"serial {name:28s} {1e3 * dt:8.1f} ms  {len(a):3d} outputs  {sum(len(x) for _, x in a):9d} bytes")
        # no output is empty, but for the probes' arrays that are empty by their models (tc.EMPTY_OUTPUTS, written out)
        empty = [label for label, x in a if len(x) == 0]
        print("".join(f"  empty: {label}\n" for label in empty), end="")
        assert len(a) > 0 and empty == tc.EMPTY_OUTPUTS.get(name, []), (name, empty)
        d = tc.first_difference(a, b)
        assert d is None, f"script {name}: output {d[0]} differs between two runs alone at byte {d[1]}"
    print(f"serial total {_serial_time(serial, serial):.2f} s")
    # the serial runs made every call the completeness table claims a script for (tests/test_thread_cases_host.py holds
    # the table against the class; a property such as source_size goes through no Log and is exempt there)
    claimed = {k for k, v in tc.COVERAGE.items() if not isinstance(v, hc.Exempt)}
    assert not claimed - serial.called, f"no serial run called {sorted(claimed - serial.called)}"
    # the scripts do what their names say
    mt = dict(serial["model_tracker"][0])
    totals = [np.frombuffer(mt[f"frame{k}.total"], np.int64).tolist() for k in range(3)]
    n_left = np.frombuffer(mt["streamed"][:8], np.int32).tolist()
    # (the box moves once, when frame 1's pose is found, and what leaves is streamed out: one list, not empty)
    assert totals == [[0, 0, 0], [-1, 0, 0], [-1, 0, 0]] and np.frombuffer(mt["shifts"], np.int32).tolist() == [1, 1], totals
    assert n_left[0] > 0 and n_left[1] == -1, n_left
    bl = dict(serial["bilateral"][0])
    assert np.frombuffer(bl["pair_after.rc"], np.int32).tolist() == [binding.E_NOT_SET]  # no frame is resident
    fb = dict(serial["align_fallback"][0])["fallback.rc"]
    assert np.frombuffer(fb, np.int32).tolist() == [binding.W_TOO_FEW_PAIRS, 2]
    st = dict(serial["align_threshold"][0])
    first, second = (int(np.frombuffer(st[k], np.int32)[0]) for k in ("kabsch.stats", "reference_on_committed.stats"))
    # the threshold ended both loops (the CPU oracle: after 11 and 4 iterations), the first one past every
    # ICPK_LOOP_AHEAD tried here
    assert 3 < first < 24 and 0 < second < 24, (first, second)
    # the fallback's get_source() agrees with the returned T: the serial reference of this session equals the CPU
    # oracle's moved source bit for bit (as test_gpu_loop_edges.py holds it), T to that test's 1e-5
    m = tc.inputs()["mid"]
    o = oracle.align(m["source"], m["target"], sum_order=1, threads=1, **m["kw"])
    got = dict(serial["align_fallback"][0])
    assert o["status"] == binding.W_TOO_FEW_PAIRS and o["iterations"] == 2
    assert got["fallback.source"] == np.ascontiguousarray(o["src_out"], np.float32).tobytes()
    Tg = np.frombuffer(got["fallback.T"], np.float32).reshape(4, 4).astype(np.float64)
    assert np.abs(Tg - o["T"].astype(np.float64)).max() < 1e-5


def test_concurrent_contexts_equal_serial(serial):
    """thread k runs scripts k, k + 1, ... (rotated, so that different families overlap at any moment), each on a fresh
    context, until every thread has run every script once"""
    _alive()
    names = [s.name for s in tc.SCRIPTS]

    def body(k):
        def run(w, barrier):
            for i in range(len(names)):
                w.fresh(names[(k + i) % len(names)])
        return run

    timeout = max(60.0, _serial_time(serial, names) * T * 4)
    workers, wall = _run_threads([body(k) for k in range(T)], timeout)
    assert _check(workers, serial, "rotated scripts", wall) == T * len(names)


def test_same_script_on_all_threads(serial):
    """identical work in lock step: where a shared staging buffer or recorder would collide"""
    _alive()
    phases = ["align_threshold", "frame_path", "batch"]

    def run(w, barrier):
        for i, name in enumerate(phases):
            if i:
                barrier.wait(timeout=60)
            w.fresh(name)

    timeout = max(60.0, _serial_time(serial, phases) * T * 4)
    workers, wall = _run_threads([run] * T, timeout)
    assert _check(workers, serial, "same script everywhere", wall) == T * len(phases)


def test_two_contexts_interleaved_on_one_thread(serial):
    """no threads: two contexts advanced call by call in alternation (shared state without timing)"""
    _alive()
    names = ["align_threshold", "prepare_chain"]
    with binding.Context(0) as a, binding.Context(0) as b:
        outs = [tc._Out(), tc._Out()]
        gens = [tc.BY_NAME[n].steps(tc.Traced(c), o) for n, c, o in zip(names, (a, b), outs)]
        steps, live = 0, list(gens)
        while live:
            for g in list(live):
                try:
                    next(g)
                    steps += 1
                except StopIteration:
                    live.remove(g)
        assert steps > 8
    for n, o in zip(names, outs):
        d = tc.first_difference(o, serial[n][0])
        assert d is None, f"interleaved with the other context, script {n}: output {d[0]} differs at byte {d[1]}"


@pytest.mark.parametrize("ahead", [None, "0", "3"])
def test_threshold_loop_under_load(serial, monkeypatch, ahead):
    """thread 0: align_threshold and align_fallback REPEATS times each on ONE context (the source uploaded anew each
    time) while 7 others run batch and frame_path ROUNDS times each (alone, 40 script runs of thread 0 take about as
    long as 2 rounds of load; 6 keeps the load running until thread 0 is through -- its overlap share says if it did)"""
    _alive()
    if ahead is None:
        monkeypatch.delenv("ICPK_LOOP_AHEAD", raising=False)
    else:
        monkeypatch.setenv("ICPK_LOOP_AHEAD", ahead)  # (read at icpk_create)
    loop, load = ["align_threshold", "align_fallback"], ["batch", "frame_path"]
    t_loop, t_load = REPEATS * _serial_time(serial, loop), _serial_time(serial, load)
    rounds = ROUNDS

    def looper(w, barrier):
        c = w.log.call("create", binding.Context, 0)
        try:
            tr = tc.Traced(c, w.log)
            for _ in range(REPEATS):
                for name in loop:
                    w.on(tr, name)
        finally:
            c.close()

    def loader(w, barrier):
        for _ in range(rounds):
            for name in load:
                w.fresh(name)

    timeout = max(60.0, max(t_loop, rounds * t_load) * T * 4)
    workers, wall = _run_threads([looper] + [loader] * (T - 1), timeout)
    n = _check(workers, serial, f"threshold loop under load, ICPK_LOOP_AHEAD={ahead}, {rounds} rounds of load", wall)
    assert n == 2 * REPEATS + (T - 1) * rounds * len(load)
    # (stats.iterations and get_source() are among the compared outputs: "*.stats", "*.source")
    assert {"kabsch.stats", "kabsch.source"} <= {label for label, _ in workers[0].results[0][1]}


# ---- the newer families ---------------------------------------------------------------------------------------------
def _same(got, label, want, what):
    assert got[label] == np.ascontiguousarray(want).tobytes(), f"{what}: output {label} is not its model's bytes"


def test_adapter_loses_nothing(serial):
    """A probe script's serial output is the probe called directly on a fresh context that goes through no Log: same
    keys, same bytes.  With threads == serial (this file) and probe == model (tests/test_gpu_history.py::
    test_fresh_probe_equals_its_model) the chain closes.  The serial bytes of `bilateral` and `tsdf_follow` are held
    against tests/bilateral_model.py and tests/tsdf_shift_model.py wherever tests/test_gpu_bilateral.py and
    tests/test_gpu_tsdf_shift.py claim bit equality."""
    _alive()
    import bilateral_model as bm
    import tsdf_mesh_model
    import tsdf_model
    import tsdf_raycast_model
    import tsdf_shift_model as sm
    from icp_slam_prototype_amd import depth, synth

    s = hc.scene("P")
    for name in tc.PROBE_SCRIPTS:
        with binding.Context(0) as c:
            want = hc.PROBES[name](c, s)
        got = serial["probe_" + name][0]
        assert [k for k, _ in got] == sorted(want), f"probe_{name}: keys {sorted(set(dict(got)) ^ set(want))}"
        for k, x in got:
            assert x == want[k], f"probe_{name}[{k}] through the adapter: {hc.first_difference(hc.blob(x), want[k])}"
    # K22
    inp = tc.inputs()
    b, got = inp["bilateral"], dict(serial["bilateral"][0])
    smooth = {}
    for r, fields in tc.BILATERAL_PARAMS:
        p = depth.bilateral_params(**fields)
        smooth[r] = bm.bilateral(b["image"], *depth.bilateral_tables(p))
        _same(got, f"radius{r}.image", smooth[r], "bilateral")
    _same(got, "radius6.in_place", smooth[6], "bilateral")
    assert smooth[1].tobytes() != smooth[6].tobytes() != np.asarray(b["image"]).tobytes()
    n = int((b["image"] != 0).sum())
    cloud = synth.backproject(smooth[1], None, b["fx"], b["cx"]) + tc.P5[:, None]
    for which in (0, 1):
        assert got[f"smoothed{which}"] == np.int32(n).tobytes() + np.ascontiguousarray(cloud, np.float32).tobytes(), which
    assert np.frombuffer(got["pair.sizes"], np.int32).tolist() == [n, n]
    # K23
    f, got = inp["tsdf_follow"], dict(serial["tsdf_follow"][0])
    fx, cx, what = f["fx"], f["cx"], "tsdf_follow"
    vol = tsdf_model.Volume(**f["volume"])
    _same(got, "fused.n", np.int32([vol.integrate(d, P, fx, cx) for d, P in f["frames"][:2]]), what)
    _same(got, "fused.tsdf", vol.tsdf, what)
    _same(got, "fused.weight", vol.weight, what)
    left = sm.leaving(vol, tc.FOLLOW_SHIFT, 1)
    _same(got, "leaving.counts", np.int32([left["points"].shape[1], left["n_no_normal"]]), what)
    for k in tc.LIST_KEYS:
        _same(got, "leaving." + k, left[k], what)
    vol = sm.shifted(vol, tc.FOLLOW_SHIFT)
    _same(got, "shifted.origin", vol.origin, what)
    _same(got, "shifted.total", vol.total, what)
    _same(got, "shifted.tsdf", vol.tsdf, what)
    _same(got, "shifted.weight", vol.weight, what)
    lo, hi = tc.FOLLOW_BOX
    sl = tuple(slice(lo[a], hi[a]) for a in (2, 1, 0))
    _same(got, "box.tsdf", vol.tsdf[sl], what)
    _same(got, "box.weight", vol.weight[sl], what)
    assert vol.weight[sl].any() and left["points"].shape[1] > 0
    d, P = f["frames"][2]
    _same(got, "third.n", np.int32(vol.integrate(d, P, fx, cx)), what)
    _same(got, "third.tsdf", vol.tsdf, what)
    _same(got, "third.weight", vol.weight, what)
    ray = tsdf_raycast_model.raycast(vol, P, **tc.FOLLOW_RAY)
    _same(got, "raycast.counts", np.int32([ray["n_hits"], ray["n_no_normal"]]), what)
    for k, maps in (("points", ray["maps"][0:3]), ("normals", ray["maps"][3:6]), ("depth", ray["maps"][6])):
        _same(got, "raycast." + k, maps, what)
    mesh = tsdf_mesh_model.mesh(vol, 1)
    _same(got, "mesh.counts", np.int32([mesh["n_vertices"], mesh["n_triangles"], mesh["n_no_normal"]]), what)
    for k in tc.MESH_ARRAYS:
        _same(got, "mesh." + k, mesh[k], what)
    srf = vol.extract(1)
    _same(got, "surface.counts", np.int32([srf["points"].shape[1], srf["n_no_normal"]]), what)
    for k in tc.LIST_KEYS:
        _same(got, "surface." + k, srf[k], what)
    assert ray["n_hits"] > 100 and mesh["n_triangles"] > 100 and srf["points"].shape[1] > 10
    _same(got, "reset.origin", np.float32(f["volume"]["origin"]), what)
    _same(got, "reset.total", np.zeros(3, np.int64), what)
    assert not np.frombuffer(got["reset.weight"], np.uint16).any()


def test_same_new_script_on_all_threads(serial):
    """identical work in lock step for the newer families: the FPFH bins, the filters' compaction, the volume and its
    second set of planes, the bilateral tables, the pose graph -- where one buffer shared by all contexts would collide"""
    _alive()
    phases = ["probe_fpfh", "probe_filter", "probe_tsdf", "tsdf_follow", "bilateral", "probe_posegraph"]

    def run(w, barrier):
        for i, name in enumerate(phases):
            if i:
                barrier.wait(timeout=60)
            w.fresh(name)

    timeout = max(60.0, _serial_time(serial, phases) * T * 4)
    workers, wall = _run_threads([run] * T, timeout)
    assert _check(workers, serial, "same new script everywhere", wall) == T * len(phases)


def _load_rounds(t_loop, t_load):
    """The rounds of (batch, frame_path) that keep the load running until thread 0 is through: ROUNDS, or more where
    this session's serial times ask for it.  Measured beside each other (the module's docstring): a round of load takes
    18 to 25 times what it takes alone (seven threads create and destroy contexts against each other), thread 0's
    probes 2 to 2.5 times; so the load outlasts thread 0 from t_loop / (7 t_load) rounds on, and t_loop / (4 t_load)
    leaves a margin of nearly two."""
    return max(ROUNDS, math.ceil(t_loop / (4 * t_load)))


def _under_load(serial, looper, t_loop, what):
    """thread 0 runs looper(worker, traced context) on ONE context while the 7 others run batch and frame_path on fresh
    ones (t_loop: what thread 0's work takes alone, seconds); returns (workers, the load's results, how many there
    must be)"""
    load = ["batch", "frame_path"]
    t_load = _serial_time(serial, load)
    rounds = _load_rounds(t_loop, t_load)

    def first(w, barrier):
        c = w.log.call("create", binding.Context, 0)
        try:
            looper(w, tc.Traced(c, w.log))
        finally:
            c.close()

    def loader(w, barrier):
        for _ in range(rounds):
            for name in load:
                w.fresh(name)

    timeout = max(60.0, max(t_loop, rounds * t_load) * T * 4)
    workers, wall = _run_threads([first] + [loader] * (T - 1), timeout)
    ends = [max((b for _, _, b in w.log.calls), default=0.0) for w in workers]
    t0 = min(a for w in workers for _, a, _ in w.log.calls)
    print(f"\n{what}: thread 0 alone {t_loop:.2f} s, a round of load alone {t_load:.3f} s, {rounds} rounds; thread 0 through "
          f"after {ends[0] - t0:.2f} s, the load after {min(ends[1:]) - t0:.2f} .. {max(ends[1:]) - t0:.2f} s")
    n = _check(workers, serial, f"{what}, {rounds} rounds of load", wall)
    return workers, n - len(workers[0].results), (T - 1) * rounds * len(load)


NEIGHBOURHOOD = ["probe_nn_grid", "probe_voxel", "probe_filter", "probe_normals", "probe_fpfh", "probe_color",
                 "probe_align_plane_to_plane", "probe_align_colored", "probe_score"]
# REPEATS cut by a factor of 4, the families kept: the nine probes take 0.115 s alone (probe_score 0.1 s of it, mostly
# the binding's 4096 information matrices on the host), so 20 repetitions are 2.3 s alone, about 5 s beside the load,
# and ask for twice the rounds of load; 5 repetitions end within the time of the file's other tests under load
NEIGHBOURHOOD_REPEATS = REPEATS // 4


def test_neighbourhood_kernels_under_load(serial):
    """The kernels whose bits must not depend on the order of arrival -- slots handed out inside a cell with atomicAdd
    (grid_qslot_kernel, morton_slot_kernel), the neighbourhood kernels that walk those cells (normals, filters, FPFH,
    colour gradients, K14's covariances), the voxel sums and the FPFH bins accumulated with atomics -- on ONE context,
    NEIGHBOURHOOD_REPEATS times over, while 7 other contexts compete for the CUs: every result is the serial bytes."""
    _alive()
    t_loop = NEIGHBOURHOOD_REPEATS * _serial_time(serial, NEIGHBOURHOOD)

    def looper(w, traced):
        for _ in range(NEIGHBOURHOOD_REPEATS):
            for name in NEIGHBOURHOOD:
                w.on(traced, name)

    workers, n_load, want_load = _under_load(serial, looper, t_loop, "neighbourhood kernels under load")
    assert len(workers[0].results) == NEIGHBOURHOOD_REPEATS * len(NEIGHBOURHOOD) and n_load == want_load
    assert [name for name, _ in workers[0].results[:len(NEIGHBOURHOOD)]] == NEIGHBOURHOOD


CHAIN = "QSPSQP"


def test_shrink_grow_chain_under_load(serial):
    """tests/test_gpu_history.py::test_shrink_grow_chain on thread 0 -- every probe of history_cases.CHAIN_PROBES on the
    scenes Q, S, P, S, Q, P on ONE context, so that every buffer is grown, left oversized and reused -- while 7 other
    contexts allocate and free.  The results on P (steps 3 and 6) are the serial bytes of probe_<name>."""
    _alive()
    names = ["probe_" + p for p in hc.CHAIN_PROBES]

    def looper(w, traced):
        for scene in CHAIN:
            for p in hc.CHAIN_PROBES:
                if scene == "P":
                    w.on(traced, "probe_" + p)
                else:
                    tc.run_probe(traced, p, scene)  # (to its end: a refusal is raised)

    # the chain alone first, on a context of its own: what it takes (the serial fixture has no times for Q and S), and
    # that it gives the serial bytes without any thread beside it
    alone = _Worker(0, None)
    with binding.Context(0) as c:
        t0 = time.perf_counter()
        looper(alone, tc.Traced(c, alone.log))
        t_loop = time.perf_counter() - t0
    for (name, got), step in zip(alone.results, (3,) * len(names) + (6,) * len(names)):
        d = tc.first_difference(got, serial[name][0])
        assert d is None, f"the chain alone, step {step}, {name}: output {d[0]} differs from the serial run at byte {d[1]}"
    workers, n_load, want_load = _under_load(serial, looper, t_loop, "shrink-grow chain under load")
    assert [name for name, _ in workers[0].results] == names * CHAIN.count("P") and n_load == want_load
    # (every probe sets the subsampling once: thread 0 did run all of them on all six scenes)
    assert sum(n == "set_subsample" for n, _, _ in workers[0].log.calls) == len(CHAIN) * len(names)


PAIRS = [("probe_fpfh", "probe_filter"), ("probe_tsdf", "tsdf_follow"), ("bilateral", "frame_path")]


@pytest.mark.parametrize("pair", PAIRS, ids=["-".join(p) for p in PAIRS])
def test_two_contexts_alternate_call_by_call(serial, pair):
    """Two threads, a context each and a baton (tc.Baton, handed over inside Log.call): exactly one library call of A is
    followed by exactly one of B and no two overlap -- shared state without timing, for the scripts that are single
    calls to test_two_contexts_interleaved_on_one_thread.  A thread whose script has ended gives the baton up for good.
    The overlap condition does not apply; instead the logged windows of the two threads must never intersect."""
    _alive()
    timeout = max(60.0, _serial_time(serial, pair) * T * 4)
    baton = tc.Baton(2, timeout)

    def body(name):
        def run(w, barrier):
            w.log.baton, w.log.who = baton, w.k
            try:
                c = w.log.call("create", binding.Context, 0)
                try:
                    w.on(tc.Traced(c, w.log), name)
                finally:
                    try:
                        w.log.call("close", c.close)
                    except tc.Stopped:
                        c.close()
            finally:
                baton.retire(w.k)
        return run

    workers, wall = _run_threads([body(n) for n in pair], timeout)
    errors = [f"thread {w.k}: {w.error}" for w in workers if w.error]
    assert not errors, "\n".join(errors)
    calls = sorted((a, b, w.k) for w in workers for _, a, b in w.log.calls)
    print(f"\nalternating {pair}: wall {wall:.2f} s, {[len(w.log.calls) for w in workers]} calls")
    for (a0, b0, k0), (a1, b1, k1) in zip(calls, calls[1:]):
        assert b0 <= a1, f"calls of threads {k0} and {k1} overlap: [{a0}, {b0}] and [{a1}, {b1}]"
    # one call of A, one of B, ... until one of the two is through
    owners = [k for _, _, k in calls]
    both = 2 * min(len(w.log.calls) for w in workers)
    assert owners[:both] == [0, 1] * (both // 2) and len(set(owners[both:])) <= 1 and both > 8
    for w, name in zip(workers, pair):
        assert [n for n, _ in w.results] == [name]
        d = tc.first_difference(w.results[0][1], serial[name][0])
        assert d is None, f"call by call beside {set(pair) - {name}}, script {name}: output {d[0]} differs at byte {d[1]}"
