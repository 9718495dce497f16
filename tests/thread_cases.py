"""Deterministic call sequences ("scripts"), one per public family, shared by tests/test_gpu_threads.py and
tests/test_thread_cases_host.py (test infrastructure; never imported by the package).

A script is `run(ctx) -> list of (label, bytes)`: it drives a FRESH context through a fixed call sequence on seeded
synth inputs and returns everything observable as bytes.  Every public result is defined to the bit, so the reference
for a script run beside other contexts on other threads is the same script run alone: any state shared between contexts
that matters shows up as a differing byte.  params.profile stays 0 everywhere (the profiling counters are per process).

`ctx` is a Traced: a binding.Context whose every call goes through its thread's Log: timed (perf_counter before and
after), named while it runs (`current`: what a hung thread was in) and refused once the shared stop event is set.
Inputs are built once, before any clock starts (inputs(); numpy and the CPU oracle's rotation helper only), so a script
is almost entirely library calls.  From the repository root,
`PYTHONPATH=.:tests python -c "import thread_cases as t; t.dry_run()"` builds them without the library and prints their
sizes.

The scripts come in three kinds.  The eleven hand-written ones of the first version.  One `probe_<name>` per probe of
tests/history_cases.py (all but `batch`, whose family the `batch` script here covers with hipMalloc through ctypes): the
probe itself, run on the Traced context on scene P, its dict as (key, bytes) in key order -- the probes already install
everything they need and return every output of one family, and tests/test_gpu_history.py holds them against the
models, so they are reused and not written a second time.  And four for what neither file reached: `bilateral` (K22),
`tsdf_follow` (K23), `model_tracker` (the TsdfVolume and ModelTracker classes) and `deferred_source` (the call
sequences of tests/test_gpu_deferred_source.py on one context).  A function that takes the context as an argument is
called as ctx.call("<name>", fn, ctx.raw, ...): the Log names it, the function gets the binding.Context itself (it
reads and sets the context's private fields).  The classes get the raw context too, and each of their methods is one
logged call.

COVERAGE maps every public name of binding.Context and the six functions over a context to the scripts that call it,
or to history_cases.EXEMPT with a reason; tests/test_thread_cases_host.py holds it against the class.
"""
import ctypes as C
import hashlib
import threading
import time

import numpy as np

import bilateral_model as bm
import history_cases as hc
import tsdf_cases as tcs
import tsdf_shift_cases as tsc
from icp_slam_prototype_amd import binding, depth, sequence, synth, tsdf

I3 = np.eye(3, dtype=np.float32)
P5 = np.full(3, 5, np.float32)  # icp.cpp:53
CAM = (5.0, 5.0, 5.0)
ROWS, COLS = 120, 160  # quarter-frame Kinect images


class Stopped(Exception):
    """another thread has failed: this one stops between two calls"""


class Baton:
    """The right to be inside a call, handed round n threads: thread k's call starts when the baton reaches k and hands
    it to the next thread that still runs when it returns, so that exactly one call of one thread is followed by exactly
    one call of the next and no two overlap.  A thread whose script has ended retires: the baton passes it by for good.
    timeout: seconds a thread waits for the baton before it gives up (the test's join time-out)."""

    def __init__(self, n, timeout):
        self.cond, self.turn, self.live, self.timeout = threading.Condition(), 0, [True] * n, timeout

    def _next(self, k):
        n = len(self.live)
        return next(((k + d) % n for d in range(1, n + 1) if self.live[(k + d) % n]), k)

    def take(self, k):
        with self.cond:
            if not self.cond.wait_for(lambda: self.turn == k, self.timeout):
                raise RuntimeError(f"thread {k}: the baton did not arrive within {self.timeout:.0f} s")

    def hand_on(self, k):
        with self.cond:
            self.turn = self._next(k)
            self.cond.notify_all()

    def retire(self, k):
        with self.cond:
            self.live[k] = False
            if self.turn == k:
                self.turn = self._next(k)
            self.cond.notify_all()


class Log:
    """One thread's record of its binding calls: calls = [(name, t0, t1)], current = the call in flight (what a hung
    thread was in).  stop: the event that, once set, refuses every further call.  baton, who: a Baton and this
    thread's place in it -- every call then waits for the baton and hands it on when it is over."""

    def __init__(self, stop=None, baton=None, who=0):
        self.calls, self.current, self.stop, self.baton, self.who = [], None, stop, baton, who

    def _stopped(self, name):
        if self.stop is not None and self.stop.is_set():
            raise Stopped(name)

    def call(self, name, fn, *a, **kw):
        self._stopped(name)
        if self.baton is None:
            return self._timed(name, fn, a, kw)
        self.baton.take(self.who)
        try:
            self._stopped(name)  # (set while this thread waited)
            return self._timed(name, fn, a, kw)
        finally:  # (after the call's window is on record: the next thread's window starts later)
            self.baton.hand_on(self.who)

    def _timed(self, name, fn, a, kw):
        self.current = name
        t0 = time.perf_counter()
        try:
            return fn(*a, **kw)
        finally:
            self.calls.append((name, t0, time.perf_counter()))
            self.current = None


class Traced:
    """binding.Context with every call made through a Log"""

    def __init__(self, ctx, log=None):
        self._ctx, self.log = ctx, log if log is not None else Log()

    @property
    def raw(self):
        """the binding.Context itself, for the functions and classes that take one (see the module's docstring)"""
        return self._ctx

    def call(self, name, fn, *a, **kw):
        return self.log.call(name, fn, *a, **kw)

    def __getattr__(self, name):
        v = getattr(self._ctx, name)
        if not callable(v):
            return v
        return lambda *a, **kw: self.log.call(name, v, *a, **kw)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def _depth_frames(n, seed, valid=0.5):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        d = synth.render_room_depth(ROWS, COLS, synth.rot_xyz_deg(0, 0.5 * k, 0.1 * k), np.array([0.01 * k, 0, 0.004 * k]),
                                    noise_sigma=0.002, rng=rng)
        d[rng.random(d.shape) > valid] = 0
        out.append(np.ascontiguousarray(d, np.uint16))
    return out


def _mid_fallback():
    """the pair of tests/test_gpu_loop_edges.py whose pair count drops below min_pairs at iteration 2 of a
    threshold-mode loop (frozen there from a search with the CPU oracle)"""
    from oracle import icp_oracle

    rng = np.random.default_rng(62)
    n = int(rng.integers(30, 300))
    tgt = rng.uniform(-1, 1, (3, n)).astype(np.float32)
    R = icp_oracle.make_rotation_matrix(*rng.uniform(-20, 20, 3)).astype(np.float64)
    src = (R @ tgt + rng.normal(0, 0.1, (3, 1)) + rng.normal(0, 0.01, (3, n))).astype(np.float32)
    kw = dict(max_iterations=16, threshold=1e-9, max_nn_dist=0.1, min_pairs=13, solve=binding.SOLVE_REFERENCE,
              last_rotation=icp_oracle.make_rotation_matrix(1.0, 2.0, 3.0), last_translation=np.float32((0.01, 0.02, -0.03)))
    return dict(source=src, target=tgt, kw=kw)


def _small_pair(seed, rows=ROWS, cols=COLS, valid=0.6):
    p = synth.kinect_pair(rows=rows, cols=cols, valid=valid, seed=seed)
    return np.ascontiguousarray(p["source"]), np.ascontiguousarray(p["target"])


# K22: the frame of several tiles (bilateral_model.TILE_CASES: 33 x 129 is three tiles by three, the last of each partly
# filled; the case has no smaller size) with two non-default parameter sets, so that the tables kept on the device change
BILATERAL_CASE = "33x129"
BILATERAL_PARAMS = ((1, dict(radius=1, sigma_space=1.0 / 1.5)), (6, dict(radius=6, sigma_space=4.0, sigma_range=45.0)))
# K23: the smallest volume of tsdf_shift_cases.CASES, `odd` (33 x 17 x 9), its frame and two further views from
# nearby; the shift has mixed signs and on the numpy models (tests/tsdf_shift_model.py) leaves 15 of the 43 crossings
# behind, 30 crossings, 332 triangles and 949 ray hits after the third frame
FOLLOW_CASE = "odd"
FOLLOW_POSES = (((20.0, 50.0, 0.0), (-0.3, 0.5, 1.1)), ((18.0, 47.0, 0.0), (-0.25, 0.5, 1.05)), ((22.0, 52.0, 0.0), (-0.3, 0.45, 1.15)))
FOLLOW_SHIFT = (-1, 1, -1)
FOLLOW_BOX = ((1, 2, 3), (30, 17, 9))
FOLLOW_RAY = dict(shape=tcs.ROOM_SHAPE, fx=tcs.ROOM_FX, cx=tcs.ROOM_CX, z_near=0.25, z_far=6.0, step=0.15, min_weight=1)
# the classes: the set-up of tests/test_gpu_tsdf_shift.py::test_tracker_follows_and_equals_where_nothing_is_lost -- the
# room volume, its first frame, follow=1 -- with that test's second frame mirrored: the camera moves 0.96 voxel towards
# -x instead of +x, so that the one shift, by (-1, 0, 0), is no lossless one (on the numpy models 48 crossings of the
# floor and the back wall leave at the volume's far side; the test's own shift by (1, 0, 0) streams nothing and its third
# frame moves the box a second time).  The third view stays 0.12 / 0.08 voxel from the new reference.  The volume is
# the room's own: a coarser voxel turns the 0.96 voxel into no shift, and in a narrower box
# (tsdf_shift_cases.WALK_VOLUME was tried on the device) the left wall is gone and the tracker drifts by centimetres
TRACKER_POSES = (((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), ((0.0, -4.0, 0.0), (-0.06, 0.0, 0.0)), ((-1.0, -3.0, 0.0), (-0.07, 0.005, 0.0)))
TRACKER_ALIGN = dict(max_iterations=20, max_nn_dist=0.1)
DEFERRED_SIZES = (65, 300)
DEFERRED_TARGET = 5_000

_INPUTS = None
_LOCK = threading.Lock()


def _new_inputs(inp):
    """the inputs of the probe scripts and of bilateral, tsdf_follow, model_tracker and deferred_source"""
    import posegraph_cases as pc
    import test_gpu_deferred_source as ds

    inp["scenes"] = {n: hc.scene(n) for n in "PQS"}  # (Q and S: test_shrink_grow_chain_under_load)
    for which in ("tgt", "src"):  # what the probes would otherwise build at their first run
        hc._full_depth(inp["scenes"]["P"], which)
    pc.case(hc.PG_CASE)
    img, _ = bm.case(BILATERAL_CASE)
    fx, cx = bm.intrinsics(120)  # (the frame is cut from the 120 x 160 room)
    inp["bilateral"] = dict(image=img, other=np.ascontiguousarray(img[::-1, ::-1]), fx=fx, cx=cx)
    assert FOLLOW_CASE in tsc.CASES
    case = tcs.case(FOLLOW_CASE)
    inp["tsdf_follow"] = dict(volume=case["volume"], fx=case["fx"], cx=case["cx"],
                              frames=[tcs.room_frame(*p) for p in FOLLOW_POSES])
    room = tcs.case("room")
    inp["tracker"] = dict(volume={k: room["volume"][k] for k in ("dims", "voxel", "origin", "trunc")}, fx=room["fx"],
                          cx=room["cx"], frames=[tcs.room_frame(*p) for p in TRACKER_POSES])
    inp["deferred"] = dict(target=ds._cloud(DEFERRED_TARGET, 100 + DEFERRED_TARGET),
                           sources={ns: (ds._cloud(ns, 200 + ns), ds._cloud(max(1, ns // 2), 300 + ns),
                                         ds._cloud(2 * ns + 7, 400 + ns)) for ns in DEFERRED_SIZES})


def build_inputs():
    """every script's inputs, built afresh (numpy only; the host test compares two builds)"""
    inp = {}
    inp["pair"] = _small_pair(501)
    inp["pair2"] = _small_pair(502, valid=0.5)
    inp["mid"] = _mid_fallback()
    inp["frames"] = _depth_frames(6, 77)
    ragged = [(120, 160), (60, 80), (96, 128), (120, 160), (40, 56)]
    inp["batch"] = [_small_pair(600 + k, r, c) for k, (r, c) in enumerate(ragged)]
    inp["streams"] = [_depth_frames(4, 900 + s) for s in range(3)]
    inp["map_frames"] = _depth_frames(5, 33, valid=1.0)
    # every 5th point of each frame, posed, in host memory: what the caller folds in with map_update_points
    inp["map_keys"] = [np.ascontiguousarray(synth.backproject(d)[:, ::5] + P5[:, None], np.float32)
                       for d in inp["map_frames"]]
    Rm, c = synth.rot_xyz_deg(0, 0.8, 0), np.array([0.02, 0.0, 0.01])
    inp["color"] = synth.render_room_color(240, 320, Rm, c, noise_sigma=2.0, rng=np.random.default_rng(4))
    inp["color_depth"] = synth.render_room_depth(240, 320, Rm, c)
    inp["tiny"] = _small_pair(700, 48, 64)
    _new_inputs(inp)
    return inp


def digest(v):
    """sha256 over everything in an inputs dict: dtypes, shapes and bytes of the arrays, repr of the rest"""
    h = hashlib.sha256()

    def walk(x):
        if isinstance(x, np.ndarray):
            h.update(f"{x.dtype}{x.shape}".encode() + np.ascontiguousarray(x).tobytes())
        elif isinstance(x, dict):
            for k in x:
                h.update(repr(k).encode())
                walk(x[k])
        elif isinstance(x, (list, tuple)):
            h.update(f"{type(x).__name__}{len(x)}".encode())
            for y in x:
                walk(y)
        else:
            h.update(repr(x).encode())

    walk(v)
    return h.hexdigest()


def inputs():
    """every script's inputs, built once (numpy only)"""
    global _INPUTS
    with _LOCK:
        if _INPUTS is None:
            _INPUTS = build_inputs()
        return _INPUTS


def dry_run():
    def size(v):
        if isinstance(v, np.ndarray):
            return f"{v.dtype}{list(v.shape)}"
        if isinstance(v, dict):
            return "{" + ", ".join(f"{k}: {size(x)}" for k, x in v.items() if isinstance(x, (np.ndarray, list, tuple, dict))) + "}"
        if isinstance(v, (list, tuple)):
            return "[" + ", ".join(size(x) for x in v) + "]"
        return type(v).__name__

    for k, v in inputs().items():
        print(f"{k:12s} {size(v)}")
    print(f"scripts ({len(SCRIPTS)}):", ", ".join(s.name for s in SCRIPTS))


# ---- what a script returns -----------------------------------------------------------------------------------------
def _stats(st):
    """iterations, status, final_pairs, final_mse, nn_launches (the rest of icpk_stats is time)"""
    return bytes(st)[:20]


def _trace(tr):
    return b"".join(it["R"].tobytes() + it["t"].tobytes() + np.int32(it["n_pairs"]).tobytes() + np.float32(it["mse"]).tobytes()
                    for it in tr)


def _robust_trace(tr):
    return b"".join(np.int32(it["kept"]).tobytes() + np.float32(it["cut"]).tobytes() + np.float64([it["c"], it["wsum"]]).tobytes()
                    for it in tr)


class _Out(list):
    def add(self, label, *parts):
        self.append((label, b"".join(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes() for p in parts)))

    def align(self, label, ctx, res, n_trace=32):
        """what one alignment leaves: T, statistics, status, trace, associations, the moved source"""
        T, st, rc = res
        self.add(label + ".T", T)
        self.add(label + ".stats", _stats(st), np.int32(rc))
        self.add(label + ".trace", _trace(ctx.get_trace(n_trace)))
        idx, dist = ctx.get_associations()
        self.add(label + ".idx", idx)
        self.add(label + ".dist", dist)
        self.add(label + ".source", ctx.get_source())


# ---- the scripts (generators: one yield per call group, for the call-by-call interleaving test) -------------------------
def align_threshold(ctx, inp, out):
    src, tgt = inp["pair"]
    ctx.set_target(tgt)
    yield
    ctx.set_source(src)
    yield
    # (thresholds from the CPU oracle's trace of this pair: the loop leaves at iteration 11 of 24, then at 4 of 24)
    res = ctx.align(max_iterations=24, threshold=5e-4, nn_mode=binding.NN_GRID, solve=binding.SOLVE_KABSCH)
    yield
    out.align("kabsch", ctx, res)
    yield
    ctx.commit_source()
    yield
    res = ctx.align(max_iterations=24, threshold=4.5e-4, nn_mode=binding.NN_GRID, solve=binding.SOLVE_REFERENCE)
    yield
    out.align("reference_on_committed", ctx, res)


def align_fallback(ctx, inp, out):
    m = inp["mid"]
    ctx.set_target(m["target"])
    ctx.set_source(m["source"])
    yield
    res = ctx.align(**m["kw"])
    out.align("fallback", ctx, res)
    T, st, rc = res
    # the fallback applies the caller's last motion to the working source: "fallback.source" of the run alone is held
    # to the CPU oracle's src_out bit for bit (test_scripts_alone_are_repeatable), every other run to the run alone
    out.add("fallback.rc", np.int32([rc, st.iterations]))


def align_fixed_hostloop(ctx, inp, out):
    src, tgt = inp["pair2"]
    ctx.set_target(tgt)
    for mode in (binding.NN_EXACT, binding.NN_PRUNED):
        ctx.set_source(src)
        yield
        res = ctx.align(max_iterations=5, fixed_iterations=1, host_loop=1, nn_mode=mode, solve=binding.SOLVE_KABSCH)
        out.align(f"hostloop.mode{mode}", ctx, res)
        yield


def frame_path(ctx, inp, out):
    frames = inp["frames"]
    ring = np.array(frames)  # this run's own frame ring: a host range can be pinned once only
    for variant in ("plain", "registered"):
        fr = frames if variant == "plain" else [ring[k] for k in range(len(frames))]
        if variant == "registered":
            ctx.register_host_buffer(ring)
        for k in range(1, len(fr)):
            # the previous frame explicitly for the first pair, then the one resident on the device (SLAM.cpp:305)
            ns, nt = ctx.backproject_pair(fr[k], fr[k - 1] if k == 1 else None, R=I3, t=P5, filter=True)
            yield
            res = ctx.align(max_iterations=16, threshold=1e-4)
            out.add(f"{variant}.frame{k}.sizes", np.int32([ns, nt]))
            out.align(f"{variant}.frame{k}", ctx, res)
            yield
        if variant == "registered":
            ctx.unregister_host_buffer(ring)


def p2l_normals_robust(ctx, inp, out):
    src, tgt = inp["pair"]
    ctx.set_target(tgt)
    ctx.set_source(src)
    yield
    ctx.estimate_target_normals(0.08, 5, CAM, keep_moments=True)
    ctx.set_robust(binding.ROBUST_TUKEY, 4.685, binding.SCALE_MEDIAN, 0.8)
    yield
    res = ctx.align(solve=binding.SOLVE_POINT_TO_PLANE, max_iterations=8, fixed_iterations=1, max_nn_dist=0.3)
    yield
    out.align("p2l", ctx, res)
    st = ctx.get_normal_stats()
    out.add("p2l.normal_stats", np.int32([st["n"], st["n_valid"]]), st["count"], st["curvature"], st["moments"])
    out.add("p2l.normals", ctx.get_target_normals())
    out.add("p2l.robust_trace", _robust_trace(ctx.get_robust_trace(32)))


def prepare_chain(ctx, inp, out):
    src, tgt = inp["pair"]
    ctx.set_target(tgt)
    yield
    ctx.set_source(src)
    yield
    for which in (1, 0):
        n = ctx.voxel_downsample(which, 0.03, binding.VOXEL_CENTROID)
        yield
        g = ctx.get_voxel_groups()
        out.add(f"voxel{which}", np.int32(n), np.int32([g["n_in"], g["n_out"]]), g["first_index"], g["count"], g["out_of_point"])
        yield
    for which, kw in ((1, dict(kind=binding.FILTER_STATISTICAL, k=12, std_ratio=1.5)),
                      (0, dict(kind=binding.FILTER_RADIUS, radius=0.08, min_neighbors=4))):
        n = ctx.remove_outliers(which, **kw)
        yield
        s = ctx.outlier_stats()
        out.add(f"filter{which}", np.int32(n), np.int32([s["n_in"], s["n_out"]]), s["value"], s["out_index"], s["summary"],
                s["kth"] if s["kth"] is not None else b"")
        yield
    out.add("filtered.target", ctx.get_target())
    yield
    out.add("filtered.source", ctx.get_source())
    yield
    res = ctx.align(max_iterations=12, threshold=1e-6, solve=binding.SOLVE_KABSCH)
    yield
    out.align("prepared", ctx, res)


_HIP = None


def hip():
    """hipMalloc / hipMemcpy / hipFree of the HIP runtime libicpk.so has mapped (tests/test_gpu_batch.py's way)"""
    global _HIP
    with _LOCK:
        if _HIP is None:
            lib = C.CDLL("libamdhip64.so")
            lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            lib.hipFree.argtypes = [C.c_void_p]
            _HIP = lib
        return _HIP


def _upload(a):
    p = C.c_void_p()
    if hip().hipMalloc(C.byref(p), max(a.nbytes, 4)) != 0 or hip().hipMemcpy(p, a.ctypes.data, a.nbytes, 1) != 0:
        raise RuntimeError("hipMalloc / hipMemcpy failed")
    return p


def batch(ctx, inp, out):
    pairs = inp["batch"]
    kw = dict(max_iterations=12, threshold=1e-6, solve=binding.SOLVE_KABSCH)
    T, st, rc, assoc = ctx.align_batch(pairs, associations=True, **kw)
    yield
    if rc < 0:
        raise binding.IcpkError(rc, "align_batch")
    out.add("batch.T", T)
    out.add("batch.stats", b"".join(_stats(s) for s in st), np.int32(rc))
    for b, (idx, dist) in enumerate(assoc):
        out.add(f"batch.assoc{b}", idx, dist)
    ptrs = []
    try:
        dev = []
        for s, t in pairs:
            ps, pt = ctx.call("hip_upload", _upload, s), ctx.call("hip_upload", _upload, t)
            ptrs += [ps, pt]
            dev.append((ps.value, s.shape[1], pt.value, t.shape[1]))
        yield
        T, st, rc = ctx.align_batch_device(dev, max_iterations=6, fixed_iterations=1)
        if rc < 0:
            raise binding.IcpkError(rc, "align_batch_device")
        out.add("batch_device.T", T)
        out.add("batch_device.stats", b"".join(_stats(s) for s in st), np.int32(rc))
        yield
        # the first pair once more as the context's own clouds, set from the same device memory (rows of a (3, n) array)
        ps, n_s, pt, n_t = dev[0]
        ctx.set_target_device(pt, pt + 4 * n_t, pt + 8 * n_t, n_t)
        ctx.set_source_device(ps, ps + 4 * n_s, ps + 8 * n_s, n_s)
        yield
        res = ctx.align(max_iterations=5, fixed_iterations=1, solve=binding.SOLVE_KABSCH)
        out.align("device_single", ctx, res)
        ctx.commit_source()
        out.add("device_single.committed", ctx.get_source())
    finally:
        for p in ptrs:
            hip().hipFree(p)


def frames_batch(ctx, inp, out):
    streams = inp["streams"]
    multi = sequence.MultiSequenceRunner(ctx, len(streams))
    for k in range(len(streams[0])):
        res = multi.step({s: streams[s][k] for s in range(len(streams))})
        yield
        for s in range(len(streams)):
            r = res[s]
            if r is not None:
                out.add(f"stream{s}.frame{k}", r["T"], np.int32([r["status"], r["iterations"]]), r["mse"], r["icp_euler"])
    for s, r in enumerate(multi.runners):
        out.add(f"stream{s}.pose", r.camera_rotation, r.camera_position)
    ctx.release_frame_streams()


def map_tracking(ctx, inp, out):
    fr, keys = inp["map_frames"], inp["map_keys"]
    ctx.set_subsample(8, 17)
    ctx.map_reset()
    # the seed (icp.cpp:47-68): the first frame's key points from host memory (ADD_CLOUD, 180), its cloud as the point list
    ctx.map_update_points(binding.MAP_ADD_CLOUD, keys[0], 180)
    yield
    ctx.backproject(fr[0], which=1)
    ctx.transform_target(I3, P5)
    ctx.map_set_points(binding.MAP_FROM_TARGET)
    yield
    for k in range(1, len(fr)):
        ctx.backproject(fr[k], which=0)
        ctx.transform_source(I3, P5)
        ctx.commit_source()
        yield
        if k % 2:
            res = ctx.align_to_map(binding.default_params(max_nn_dist=0.1, max_iterations=10, threshold=1e-5), delta=25)
        else:
            res = ctx.align_to_map_dense(binding.default_params(max_nn_dist=0.75, max_iterations=10, threshold=1e-5), delta=25)
        yield
        out.align(f"map.frame{k}", ctx, res)
        # the frame's own key points, uploaded from host memory between two alignments
        ctx.map_update_points(binding.MAP_ADD_UNASSOCIATED, keys[k], 25)
        yield
        for lst in (binding.MAP_KEYPOINTS, binding.MAP_POINTS):
            out.add(f"map.frame{k}.list{lst}", np.int32(ctx.map_size(lst)), ctx.map_get_list(lst))
    ctx.map_release()


def fast(ctx, inp, out):
    kp, resp = ctx.detect_fast(inp["color"])
    yield
    out.add("fast.kp", kp, resp, np.int32(ctx.detected_count))
    n = ctx.detected_to_cloud(inp["color_depth"], R=I3, t=P5, which=0)
    out.add("fast.cloud", np.int32(n), ctx.get_source())


def lifecycle(ctx, inp, out):
    """icpk_create, one small alignment, icpk_destroy; five times over (the script's own context stays idle)"""
    src, tgt = inp["tiny"]
    for k in range(5):
        c = ctx.call("create", binding.Context, 0)
        try:
            ctx.call("lc.set_target", c.set_target, tgt)
            ctx.call("lc.set_source", c.set_source, src)
            T, st, rc = ctx.call("lc.align", c.align, max_iterations=4 + k, threshold=1e-6)
            out.add(f"life{k}", T, _stats(st), np.int32(rc), ctx.call("lc.get_source", c.get_source))
        finally:
            ctx.call("close", c.close)
        yield


# ---- the probes of tests/history_cases.py as scripts -----------------------------------------------------------------
def run_probe(ctx, name, scene):
    """probe `name` on the Traced context on scene "P", "Q" or "S": its dict"""
    return hc.PROBES[name](ctx, inputs()["scenes"][scene])


def _probe_script(name):
    def fn(ctx, inp, out):
        res = hc.PROBES[name](ctx, inp["scenes"]["P"])
        out.extend((k, bytes(res[k])) for k in sorted(res))
        yield

    fn.__name__ = "probe_" + name
    return fn


PROBE_SCRIPTS = tuple(k for k in hc.PROBE_ORDER if k != "batch")  # (`batch` hands torch's device memory over: see above)
# A hand-written script returns no empty output; a probe returns every array of its family, and on scene P these are
# empty (tests/test_gpu_history.py holds the probes against their models): the map's point list before map_set_points
# has filled it, and the list of key points associate_keypoints rejected, of which P has none
EMPTY_OUTPUTS = {"probe_map": ["filled.points"], "probe_frontend": ["kp.rejected"]}


# ---- K22, K23, the classes, the deferred source ----------------------------------------------------------------------
LIST_KEYS = ("points", "normals", "intensity", "voxel", "axis")
MESH_ARRAYS = ("vertices", "normals", "intensity", "voxel_index", "edge", "triangles")
RAY_MAPS = ("points", "normals", "depth")


def bilateral(ctx, inp, out):
    b = inp["bilateral"]
    img, other, fx, cx, raw = b["image"], b["other"], b["fx"], b["cx"], ctx.raw
    # a frame made resident first: the filter shares its image buffers, so none may be resident afterwards
    out.add("pair.sizes", np.int32(ctx.backproject_pair(img, other, fx=fx, cx=cx)))
    yield
    params = {r: depth.bilateral_params(**fields) for r, fields in BILATERAL_PARAMS}
    for r, p in params.items():  # (radius 1, then 6: the tables kept on the device are replaced)
        out.add(f"radius{r}.image", ctx.call("bilateral_depth_image", depth.bilateral_depth_image, raw, img, p))
        yield
    buf = np.array(img)
    ctx.call("bilateral_depth_image", depth.bilateral_depth_image, raw, buf, params[6], out=buf)
    out.add("radius6.in_place", buf)
    yield
    for which in (0, 1):  # (radius 1 again)
        n = ctx.call("backproject_smoothed", depth.backproject_smoothed, raw, img, which=which, fx=fx, cx=cx, offset=P5,
                     params=params[1])
        yield
        out.add(f"smoothed{which}", np.int32(n), ctx.get_source() if which == 0 else ctx.get_target())
        yield
    n = ctx.call("backproject_smoothed", depth.backproject_smoothed, raw, img, which=1, normals_mode=binding.NORMALS_CROSS,
                 fx=fx, cx=cx, params=params[6])
    yield
    out.add("smoothed_normals", np.int32(n), ctx.get_target(), ctx.get_target_normals())
    yield
    try:
        ctx.backproject_pair(other, None, fx=fx, cx=cx)
        rc = binding.OK
    except binding.IcpkError as e:
        rc = e.code
    out.add("pair_after.rc", np.int32(rc))


def _planes(out, label, ctx):
    f, w, _ = ctx.tsdf_get()
    out.add(label + ".tsdf", f)
    out.add(label + ".weight", w)


def _origin(out, label, ctx):
    p, total = ctx.call("tsdf_get_params", binding.tsdf_get_params, ctx.raw)
    out.add(label + ".origin", np.float32(p.origin[:]))
    out.add(label + ".total", total)


def tsdf_follow(ctx, inp, out):
    f, raw = inp["tsdf_follow"], ctx.raw
    v, fx, cx, frames = f["volume"], f["fx"], f["cx"], f["frames"]
    ctx.tsdf_create(dims=v["dims"], voxel=v["voxel"], origin=v["origin"], trunc=v["trunc"])
    yield
    n = []
    for d, P in frames[:2]:
        n.append(ctx.tsdf_integrate(d, P, fx=fx, cx=cx))
        yield
    out.add("fused.n", np.int32(n))
    _planes(out, "fused", ctx)
    yield
    out.add("leaving.counts", np.int32(ctx.call("tsdf_extract_leaving", binding.tsdf_extract_leaving, raw, FOLLOW_SHIFT, 1)))
    yield
    left = ctx.tsdf_get_surface()
    for k in LIST_KEYS:
        out.add("leaving." + k, left[k])
    yield
    ctx.call("tsdf_shift", binding.tsdf_shift, raw, FOLLOW_SHIFT)
    yield
    _origin(out, "shifted", ctx)
    _planes(out, "shifted", ctx)
    yield
    bf, bw, _ = ctx.call("tsdf_get_box", binding.tsdf_get_box, raw, *FOLLOW_BOX)
    out.add("box.tsdf", bf)
    out.add("box.weight", bw)
    yield
    d, P = frames[2]
    out.add("third.n", np.int32(ctx.tsdf_integrate(d, P, fx=fx, cx=cx)))
    _planes(out, "third", ctx)
    yield
    out.add("raycast.counts", np.int32(ctx.tsdf_raycast(P, **FOLLOW_RAY)))
    yield
    ray = ctx.tsdf_get_raycast()
    for k in RAY_MAPS:
        out.add("raycast." + k, ray[k])
    yield
    out.add("mesh.counts", np.int32(ctx.tsdf_extract_mesh(1)))
    yield
    mesh = ctx.tsdf_get_mesh()
    for k in MESH_ARRAYS:
        out.add("mesh." + k, mesh[k])
    yield
    out.add("surface.counts", np.int32(ctx.tsdf_extract_surface(1)))
    yield
    surface = ctx.tsdf_get_surface()
    for k in LIST_KEYS:
        out.add("surface." + k, surface[k])
    yield
    ctx.tsdf_reset()  # (the box is back where it was created, and empty)
    _origin(out, "reset", ctx)
    out.add("reset.weight", ctx.tsdf_get(tsdf=False)[1])
    ctx.tsdf_release()


def model_tracker(ctx, inp, out):
    """tsdf.TsdfVolume and tsdf.ModelTracker on the raw context; each of their methods is one logged call"""
    m = inp["tracker"]
    v = m["volume"]
    vol = ctx.call("TsdfVolume", tsdf.TsdfVolume, ctx.raw, dims=v["dims"], voxel=v["voxel"], origin=v["origin"],
                   trunc=v["trunc"], fx=m["fx"], cx=m["cx"])
    left = []
    tracker = tsdf.ModelTracker(vol, pose=m["frames"][0][1], z_near=0.25, z_far=6.0, step=0.125, bilateral=True, follow=1,
                                on_leave=left.append, **TRACKER_ALIGN)
    yield
    for k, (d, _) in enumerate(m["frames"]):
        pose = ctx.call("ModelTracker.track", tracker.track, d)
        out.add(f"frame{k}.pose", pose)
        out.add(f"frame{k}.total", vol.total)
        yield
    out.add("shifts", np.int32([tracker.shifts, len(left)]))
    f, w, _ = ctx.call("TsdfVolume.planes", vol.planes)
    out.add("planes.tsdf", f)
    out.add("planes.weight", w)
    yield
    out.add("streamed", np.int32([s["points"].shape[1] for s in left] + [-1]),
            *[s[k] for s in left for k in ("points", "normals", "voxel", "axis")])
    surface = ctx.call("TsdfVolume.surface", vol.surface, 1)
    for k in LIST_KEYS:
        out.add("surface." + k, surface[k])
    yield
    ctx.call("TsdfVolume.release", vol.release)


def _flat(x):
    """what tests/test_gpu_deferred_source.py::_play returns (nested lists and tuples of bytes and numbers) as bytes"""
    if isinstance(x, (bytes, bytearray)):
        return bytes(x)
    if isinstance(x, (list, tuple)):
        return b"".join(_flat(y) for y in x)
    return np.asarray(x).tobytes()


def deferred_source(ctx, inp, out):
    """the twelve call sequences of tests/test_gpu_deferred_source.py on ONE context, which defers the copy of the
    committed source wherever it can, at both source sizes against the one target"""
    import test_gpu_deferred_source as ds

    d = inp["deferred"]
    ctx.set_target(d["target"])
    yield
    for ns, (src, small, large) in d["sources"].items():
        for name, ops in ds._sequences(src, small, large).items():
            out.add(f"n{ns}.{name}", _flat(ds._play(ctx, [("set", src)] + ops, eager=False)))
            yield


class Script:
    def __init__(self, fn):
        self.name, self.fn = fn.__name__, fn

    def steps(self, ctx, out):
        """the script as a generator that yields between calls; out: the _Out it fills"""
        return self.fn(ctx, inputs(), out)

    def run(self, ctx):
        out = _Out()
        for _ in self.steps(ctx, out):
            pass
        return out


SCRIPTS = [Script(f) for f in (align_threshold, align_fallback, align_fixed_hostloop, frame_path, p2l_normals_robust,
                               prepare_chain, batch, frames_batch, map_tracking, fast, lifecycle)]
SCRIPTS += [Script(_probe_script(k)) for k in PROBE_SCRIPTS]
SCRIPTS += [Script(f) for f in (bilateral, tsdf_follow, model_tracker, deferred_source)]
BY_NAME = {s.name: s for s in SCRIPTS}


# ---- the completeness table -----------------------------------------------------------------------------------------
# the functions over a context that are no methods of binding.Context (K22: depth.py, K23: binding.py)
MODULE_FUNCTIONS = {"bilateral_depth_image": depth.bilateral_depth_image, "backproject_smoothed": depth.backproject_smoothed,
                    "tsdf_shift": binding.tsdf_shift, "tsdf_extract_leaving": binding.tsdf_extract_leaving,
                    "tsdf_get_params": binding.tsdf_get_params, "tsdf_get_box": binding.tsdf_get_box}
_RCCL = ("two communicators in one process are outside the threading claim; tests/test_gpu_comm.py and "
         "tests/test_gpu_comm_two_ranks.py own the RCCL calls")
RCCL_NAMES = ("align_query_sharded", "comm_init", "comm_destroy", "comm_rank", "comm_world", "comm_broadcast_target",
              "comm_gather_results", "comm_allreduce_sums", "comm_barrier")
# what no probe script calls: the names history_cases.COVERAGE gives to its `batch` probe or to an early path alone, and
# the six functions (tests/test_thread_cases_host.py reads each listed script's text for the call)
HAND_WRITTEN = {
    "set_target_device": ("batch",), "set_source_device": ("batch",), "align_batch": ("batch",), "align_batch_device": ("batch",),
    "commit_source": ("align_threshold", "map_tracking", "batch"),
    "align_frames_batch": ("frames_batch",), "get_frames_trace": ("frames_batch",), "release_frame_streams": ("frames_batch",),
    "transform_target": ("map_tracking",), "map_release": ("map_tracking",),
    "tsdf_reset": ("tsdf_follow",), "tsdf_release": ("tsdf_follow",),
    "bilateral_depth_image": ("bilateral",), "backproject_smoothed": ("bilateral",),
    "tsdf_shift": ("tsdf_follow",), "tsdf_extract_leaving": ("tsdf_follow",), "tsdf_get_params": ("tsdf_follow",),
    "tsdf_get_box": ("tsdf_follow",),
}


def _coverage():
    """history_cases.COVERAGE's names and exemptions; a name a probe calls is covered through probe_<name> (derived,
    not listed again); the rest from HAND_WRITTEN.  A name that ends with no script fails the host test."""
    cov = {}
    for name, users in hc.COVERAGE.items():
        if isinstance(users, hc.Exempt):
            cov[name] = users
        elif name in RCCL_NAMES:
            cov[name] = hc.EXEMPT(_RCCL)
        else:
            cov[name] = tuple("probe_" + u for u in users if u in PROBE_SCRIPTS) + HAND_WRITTEN.get(name, ())
    for name in MODULE_FUNCTIONS:
        cov[name] = HAND_WRITTEN.get(name, ())
    return cov


COVERAGE = _coverage()


def first_difference(a, b):
    """None if two script results are byte-equal, else (label, index of the first differing byte or 'length')"""
    if [l for l, _ in a] != [l for l, _ in b]:
        return ("labels", 0)
    for (label, x), (_, y) in zip(a, b):
        if x != y:
            if len(x) != len(y):
                return (label, f"length {len(x)} != {len(y)}")
            d = np.flatnonzero(np.frombuffer(x, np.uint8) != np.frombuffer(y, np.uint8))
            return (label, int(d[0]))
    return None
