"""The device loop's outputs as they reach the host: icpk_get_trace and the statistics of icpk_align's device loop
against the host loop, which keeps its trace on the host and never goes through the mirror.

The loop step stores nothing in host memory while it iterates; the step that ends the loop copies the trace of the
completed iterations into the mirror together with the result.  Every way out of the loop is covered: the loop test
(fixed iterations 1, 2 and 20; threshold mode leaving after a few iterations, enqueued whole and throttled), the
min_pairs fallback, max_iterations = 0 (the statistics-only step) and the robust flavour, whose own trace keeps
going to pinned memory entry by entry.

Reference and Kabsch flavours: bit for bit.  Point-to-plane: 1e-5 on T and on every trace entry, as the project
compares that flavour elsewhere; counts exactly.  Clouds of 2025 points on a wavy surface with analytic normals."""
import numpy as np
import pytest

from icp_slam_prototype_amd import binding

pytestmark = pytest.mark.gpu

FLAVOURS = {"reference": binding.SOLVE_REFERENCE, "kabsch": binding.SOLVE_KABSCH, "p2l": binding.SOLVE_POINT_TO_PLANE}


def _rot(ax, ay, az):
    ax, ay, az = np.radians([ax, ay, az])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


@pytest.fixture(scope="module")
def clouds():
    u, v = np.meshgrid(np.linspace(-1.0, 1.0, 45), np.linspace(-0.8, 0.8, 45))
    u, v = u.ravel(), v.ravel()
    z = 0.15 * np.sin(2.1 * u) * np.cos(1.7 * v) + 0.05 * u * v
    zu = 0.15 * 2.1 * np.cos(2.1 * u) * np.cos(1.7 * v) + 0.05 * v
    zv = -0.15 * 1.7 * np.sin(2.1 * u) * np.sin(1.7 * v) + 0.05 * u
    tgt = np.stack([u, v, z]) + 5.0
    nrm = np.stack([-zu, -zv, np.ones_like(u)])
    nrm /= np.linalg.norm(nrm, axis=0, keepdims=True)
    c = tgt.mean(1, keepdims=True)
    src = _rot(0.8, -0.6, 0.7) @ (tgt - c) + c + np.array([[0.015], [-0.01], [0.008]])
    # (a larger motion, more than a grid spacing: the associations, and with them the error, settle over several iterations)
    far = _rot(3.0, -2.5, 4.0) @ (tgt - c) + c + np.array([[0.05], [-0.04], [0.03]])
    return dict(src=src.astype(np.float32), src_far=far.astype(np.float32), tgt=tgt.astype(np.float32),
                nrm=nrm.astype(np.float32))


@pytest.fixture(scope="module")
def ctx():
    from icp_slam_prototype_amd import build

    build.build()
    with binding.Context(0) as c:
        yield c


def _load(ctx, clouds):
    ctx.set_target(clouds["tgt"])
    ctx.set_target_normals(clouds["nrm"])
    ctx.set_source(clouds["src"])


def _run(ctx, **kw):
    T, st, rc = ctx.align(nn_mode=binding.NN_GRID, **kw)
    idx, dist = ctx.get_associations()
    return dict(T=T.copy(), rc=rc, iterations=st.iterations, status=st.status, final_pairs=st.final_pairs,
                final_mse=np.float32(st.final_mse), idx=idx, dist=dist, src=ctx.get_source().copy(),
                trace=ctx.get_trace(max_iterations=64))


def _compare(dev, host, what, exact):
    for k in ("rc", "iterations", "status", "final_pairs"):
        assert dev[k] == host[k], (what, k, dev[k], host[k])
    assert len(dev["trace"]) == len(host["trace"]), (what, len(dev["trace"]), len(host["trace"]))
    assert [e["n_pairs"] for e in dev["trace"]] == [e["n_pairs"] for e in host["trace"]], what
    assert np.array_equal(dev["idx"], host["idx"]), what
    if exact:
        assert dev["final_mse"].tobytes() == host["final_mse"].tobytes(), what
        for k in ("T", "dist", "src"):
            assert dev[k].tobytes() == host[k].tobytes(), (what, k)
        for i, (a, b) in enumerate(zip(dev["trace"], host["trace"])):
            assert a["R"].tobytes() == b["R"].tobytes() and a["t"].tobytes() == b["t"].tobytes(), (what, i)
            assert a["mse"].tobytes() == b["mse"].tobytes(), (what, i)
    else:
        assert np.linalg.norm(dev["T"].astype(np.float64) - host["T"]) < 1e-5, what
        assert abs(float(dev["final_mse"]) - float(host["final_mse"])) < 1e-5, what
        for i, (a, b) in enumerate(zip(dev["trace"], host["trace"])):
            assert np.linalg.norm(a["R"].astype(np.float64) - b["R"]) < 1e-5, (what, i)
            assert np.linalg.norm(a["t"].astype(np.float64) - b["t"]) < 1e-5, (what, i)
            assert abs(float(a["mse"]) - float(b["mse"])) < 1e-5, (what, i)


def _both(ctx, what, exact, **kw):
    dev = _run(ctx, host_loop=0, **kw)
    host = _run(ctx, host_loop=1, **kw)
    _compare(dev, host, what, exact)
    return dev


@pytest.mark.parametrize("iterations", [1, 2, 20])
@pytest.mark.parametrize("flavour", ["reference", "kabsch", "p2l"])
def test_fixed_iterations(ctx, clouds, flavour, iterations):
    _load(ctx, clouds)
    r = _both(ctx, (flavour, iterations), flavour != "p2l", solve=FLAVOURS[flavour], max_iterations=iterations,
              fixed_iterations=1, max_nn_dist=0.3)
    assert r["rc"] == 0 and r["iterations"] == len(r["trace"]) == iterations and r["final_pairs"] > 1000


@pytest.mark.parametrize("ahead", ["0", "1"])
@pytest.mark.parametrize("flavour", ["reference", "kabsch", "p2l"])
def test_threshold_exit_after_a_few_iterations(monkeypatch, clouds, flavour, ahead):
    """A loop that leaves at its test after a few of its 20 iterations: enqueued whole (ICPK_LOOP_AHEAD=0, nothing
    watches the progress words) and throttled (1, the host follows them)."""
    monkeypatch.setenv("ICPK_LOOP_AHEAD", ahead)
    with binding.Context(0) as c:  # (the knob is read when the context is made)
        _load(c, clouds)
        c.set_source(clouds["src_far"])
        kw = dict(solve=FLAVOURS[flavour], max_nn_dist=0.3)
        full = _run(c, host_loop=1, max_iterations=20, fixed_iterations=1, **kw)
        mse = [float(e["mse"]) for e in full["trace"]]
        # the last of iterations 2 .. 6 in front of which the error is lower than ever before: a threshold half way
        # down to it makes that iteration's test the first to fail
        k = max(i for i in range(2, 7) if mse[i] < min(mse[:i]))
        threshold = 0.5 * (mse[k] + min(mse[:k]))
        r = _both(c, (flavour, ahead), flavour != "p2l", max_iterations=20, threshold=threshold, **kw)
        assert r["rc"] == 0 and r["iterations"] == len(r["trace"]) == k


@pytest.mark.parametrize("flavour", ["reference", "kabsch", "p2l"])
def test_min_pairs_fallback(ctx, clouds, flavour):
    """min_pairs above the pair count: no solve, the caller's last motion, an empty trace."""
    _load(ctx, clouds)
    last_R = _rot(0.2, 0.1, -0.3).astype(np.float32)
    last_t = np.array([0.004, -0.002, 0.001], np.float32)
    r = _both(ctx, flavour, flavour != "p2l", solve=FLAVOURS[flavour], max_iterations=5, fixed_iterations=1,
              max_nn_dist=0.3, min_pairs=clouds["src"].shape[1] + 1, last_rotation=last_R, last_translation=last_t)
    assert r["rc"] == r["status"] == binding.W_TOO_FEW_PAIRS and r["iterations"] == 0 and r["trace"] == []
    assert r["final_pairs"] > 1000


@pytest.mark.parametrize("flavour", ["reference", "kabsch", "p2l"])
def test_max_iterations_zero(ctx, clouds, flavour):
    """One sweep and the statistics-only step: the result is published with an empty trace."""
    _load(ctx, clouds)
    r = _both(ctx, flavour, flavour != "p2l", solve=FLAVOURS[flavour], max_iterations=0, fixed_iterations=1, max_nn_dist=0.3)
    assert r["rc"] == 0 and r["iterations"] == 0 and r["trace"] == [] and r["final_pairs"] > 1000
    assert np.array_equal(r["T"], np.eye(4, dtype=np.float32)) and r["src"].tobytes() == clouds["src"].tobytes()


def test_robust_trace_untouched(ctx, clouds):
    """The robust flavour writes its own trace into pinned memory entry by entry, as before."""
    _load(ctx, clouds)
    ctx.set_robust(binding.ROBUST_HUBER, 0.02, binding.SCALE_FIXED, 0.9)
    try:
        kw = dict(solve=binding.SOLVE_KABSCH, max_iterations=6, fixed_iterations=1, max_nn_dist=0.3)
        dev = _run(ctx, host_loop=0, **kw)
        rdev = ctx.get_robust_trace()
        host = _run(ctx, host_loop=1, **kw)
        rhost = ctx.get_robust_trace()
    finally:
        ctx.set_robust(None)
    _compare(dev, host, "robust", True)
    assert dev["iterations"] == len(dev["trace"]) == len(rdev) == 6 and rdev == rhost
    assert all(0 < e["kept"] <= t["n_pairs"] for e, t in zip(rdev, dev["trace"]))
