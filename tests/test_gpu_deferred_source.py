"""icpk_set_source / icpk_reset_source leave the copy of the committed source into the working one to whoever reads the
working planes first; a device loop of grid sweeps never does.  Every sequence below runs on ONE context, which defers
wherever it can, and on a fresh context that never defers -- it calls get_source right after every set_source /
reset_source, which makes the copy there and then -- and the two must agree byte for byte in everything they return:
transform, statistics, trace, associations, source.

Source sizes 1, 63, 64, 65, 300 (around the 64-point tile and wave) and 70 000 (a canonical lane holds two terms, the
sweep's last wave is partial); targets of 1 and 5 000 points."""
import numpy as np
import pytest

from icp_slam_prototype_amd import binding

pytestmark = pytest.mark.gpu

SOURCE_SIZES = [1, 63, 64, 65, 300, 70_000]
TARGET_SIZES = [1, 5_000]
R_MOVE = np.array([[0.9998, -0.0175, 0.01], [0.0174, 0.9998, 0.0087], [-0.0101, -0.0085, 0.9999]], np.float32)
T_MOVE = np.array([0.01, -0.02, 0.015], np.float32)
ALIGN = dict(max_iterations=3, fixed_iterations=1, solve=binding.SOLVE_KABSCH)


def _cloud(n, seed):
    rng = np.random.default_rng(seed)
    return (5.0 + 0.4 * rng.random((3, n))).astype(np.float32)


def _align(ctx, **kw):
    T, st, rc = ctx.align(**{**ALIGN, **kw})
    tr = ctx.get_trace()
    return [T.tobytes(), (rc, st.iterations, st.status, st.final_pairs, np.float32(st.final_mse).tobytes()),
            [(e["R"].tobytes(), e["t"].tobytes(), e["n_pairs"], e["mse"].tobytes()) for e in tr]]


def _assoc(ctx):
    idx, dist = ctx.get_associations()
    return [idx.tobytes(), dist.tobytes()]


def _play(ctx, ops, eager):
    """ops on ctx, everything they return in order.  eager: the working source is read back right after every
    set_source / reset_source, so that nothing is left deferred."""
    out = []
    for op, *a in ops:
        if op == "set":
            ctx.set_source(a[0])
        elif op == "reset":
            ctx.reset_source()
        elif op == "get":
            out.append(ctx.get_source().tobytes())
        elif op == "assoc":
            out.append(_assoc(ctx))
        elif op == "align":
            out.append(_align(ctx, **a[0]))
        elif op == "nn":
            idx, dist = ctx.nn(a[0])
            out.append([idx.tobytes(), dist.tobytes()])
        elif op == "transform":
            ctx.transform_source(R_MOVE, T_MOVE)
        elif op == "commit":
            ctx.commit_source()
        if eager and op in ("set", "reset"):
            ctx.get_source()
    return out


GRID = dict(nn_mode=binding.NN_GRID)


def _sequences(src, small, large):
    return {
        "set-get": [("get",)],
        "reset-get": [("reset",), ("get",)],
        "reset-align-get-assoc": [("reset",), ("align", GRID), ("get",), ("assoc",)],
        "reset-nn-exact": [("reset",), ("nn", binding.NN_EXACT), ("get",)],
        "reset-nn-filtered": [("reset",), ("nn", binding.NN_FILTERED), ("get",)],
        "reset-nn-pruned": [("reset",), ("nn", binding.NN_PRUNED), ("get",)],
        "reset-transform-align": [("reset",), ("transform",), ("get",), ("align", GRID), ("get",), ("assoc",)],
        "reset-align-host-loop": [("reset",), ("align", dict(host_loop=1, **GRID)), ("get",), ("assoc",)],
        "align-reset-reset-align": [("align", GRID), ("reset",), ("reset",), ("align", GRID), ("assoc",), ("get",)],
        "smaller-then-larger": [("align", GRID), ("set", small), ("align", GRID), ("get",), ("set", large), ("align", GRID),
                                ("assoc",), ("get",), ("set", src), ("reset",), ("get",)],
        "reset-commit": [("reset",), ("commit",), ("get",), ("align", GRID), ("get",), ("reset",), ("get",)],
        "exact-then-grid": [("reset",), ("align", dict(nn_mode=binding.NN_EXACT)), ("align", GRID), ("get",), ("assoc",)],
    }


@pytest.fixture(scope="module")
def lib():
    from icp_slam_prototype_amd import build

    build.build()


@pytest.mark.parametrize("nt", TARGET_SIZES)
@pytest.mark.parametrize("ns", SOURCE_SIZES)
def test_deferred_source_equals_eager_source(lib, ns, nt):
    tgt = _cloud(nt, 100 + nt)
    src = _cloud(ns, 200 + ns)
    small = _cloud(max(1, ns // 2), 300 + ns)
    large = _cloud(2 * ns + 7, 400 + ns)
    with binding.Context(0) as subject:
        subject.set_target(tgt)
        for name, ops in _sequences(src, small, large).items():
            ops = [("set", src)] + ops
            got = _play(subject, ops, eager=False)
            with binding.Context(0) as fresh:
                fresh.set_target(tgt)
                want = _play(fresh, ops, eager=True)
            assert len(got) == len(want)
            for k, (g, w) in enumerate(zip(got, want)):
                assert g == w, (ns, nt, name, k)
            if name == "set-get":
                assert got[0] == src.tobytes()
