"""The real loop (icpk_align: device loop and host loop, both NN modes, both solve flavours) on degenerate geometry and
at the min_pairs fallback (icp.cpp:163-182), against each other bit for bit and against the CPU oracle.

Geometry: exactly collinear and exactly planar clouds, a mirror-image target (det H < 0) and a cube lattice (isotropic
covariance), noise-free, at (5, 5, 5) and at 10^4 m.  min_pairs: 3- and 4-point clouds at min_pairs 1..5 (exactly
min_pairs pairs solve, one fewer falls back), min_pairs < 1 refused with ICPK_E_ARG, and a fallback in the MIDDLE of a threshold-mode loop for every
ICPK_LOOP_AHEAD, alone and inside a frame batch."""
import numpy as np
import pytest

from icp_slam_prototype_amd import binding, synth

pytestmark = pytest.mark.gpu

OFFSETS = {"near": np.array([5.0, 5.0, 5.0]), "far": np.array([1e4, 1e4, 1e4])}


@pytest.fixture(scope="module")
def ctx():
    from icp_slam_prototype_amd import build

    build.build()
    c = binding.Context(0)
    yield c
    c.close()


def _cloud(kind, off):
    g = np.arange(-3, 4, dtype=np.float64) * 0.1
    if kind == "collinear":
        t = np.arange(-40, 41, dtype=np.float64) * 0.02
        P = np.outer([0.6, 0.0, 0.8], t)
    elif kind == "planar":
        u, v = np.meshgrid(np.arange(-8, 9) * 0.05, np.arange(-6, 7) * 0.05)
        P = np.stack([u.ravel(), v.ravel(), np.zeros(u.size)])
    elif kind in ("cube", "mirror"):
        P = np.stack(np.meshgrid(g, g, g)).reshape(3, -1)
        if kind == "mirror":  # an asymmetric set, so that its mirror image is no rotation of it
            P = P[:, (P[0] + 2 * P[1] + 3 * P[2] > -0.35)]
    return P + off[:, None]


def _pair(kind, off):
    P = _cloud(kind, off)
    c = P.mean(1, keepdims=True)
    Rm = _rot(0.5, -0.3, 0.4)
    src = Rm @ (P - c) + c + np.array([[0.012], [-0.008], [0.005]])
    tgt = P.copy()
    if kind == "mirror":
        tgt[0] = 2 * c[0, 0] - tgt[0]
    return src.astype(np.float32), tgt.astype(np.float32)


def _rot(ax, ay, az):
    ax, ay, az = np.radians([ax, ay, az])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _run(ctx, src, tgt, **kw):
    ctx.set_target(tgt)
    ctx.set_source(src)
    T, st, rc = ctx.align(**kw)
    idx, dist = ctx.get_associations()
    return dict(T=T.copy(), rc=rc, iterations=st.iterations, status=st.status, final_pairs=st.final_pairs,
                final_mse=st.final_mse, idx=idx.copy(), dist=dist.copy(), src=ctx.get_source().copy(),
                trace=ctx.get_trace())


def _assert_same_run(a, b, what):
    for k in ("rc", "iterations", "status", "final_pairs"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    assert np.float32(a["final_mse"]).view(np.uint32) == np.float32(b["final_mse"]).view(np.uint32), what
    for k in ("T", "dist", "src"):
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint32), np.ascontiguousarray(b[k]).view(np.uint32)), (what, k)
    assert np.array_equal(a["idx"], b["idx"]), what
    assert len(a["trace"]) == len(b["trace"]) == a["iterations"], what
    for ta, tb in zip(a["trace"], b["trace"]):
        assert np.array_equal(ta["R"].view(np.uint32), tb["R"].view(np.uint32)), what
        assert np.array_equal(ta["t"].view(np.uint32), tb["t"].view(np.uint32)), what
        assert ta["n_pairs"] == tb["n_pairs"] and np.float32(ta["mse"]) == np.float32(tb["mse"]), what


def _T_close(T, oT, tol=1e-5):
    """Rotation block within 1e-5 Frobenius, absolute; translation within 1e-5 relative to its own size (about 150 at
    the far offset, where float32 positions carry 1e-3 m)."""
    T, oT = np.asarray(T, np.float64), np.asarray(oT, np.float64)
    if not float(np.linalg.norm(T[:3, :3] - oT[:3, :3])) < tol:
        return False
    return float(np.linalg.norm(T[:3, 3] - oT[:3, 3])) < tol * max(1.0, float(np.abs(oT[:3, 3]).max()))


@pytest.mark.parametrize("where", ["near", "far"])
@pytest.mark.parametrize("kind", ["collinear", "planar", "mirror", "cube"])
def test_degenerate_geometry_device_loop_equals_host_loop_and_oracle(ctx, oracle, kind, where):
    src, tgt = _pair(kind, OFFSETS[where])
    for solve in (binding.SOLVE_REFERENCE, binding.SOLVE_KABSCH):
        o = oracle.align(src, tgt, max_iterations=8, threshold=1e-12, solve=solve, sum_order=1,
                         threads=oracle.max_threads())
        for mode in (binding.NN_EXACT, binding.NN_GRID):
            runs = [_run(ctx, src, tgt, solve=solve, nn_mode=mode, host_loop=h, max_iterations=8, threshold=1e-12)
                    for h in (0, 1)]
            what = (kind, where, solve, mode)
            _assert_same_run(runs[0], runs[1], what)
            r = runs[0]
            assert (r["status"], r["iterations"], r["final_pairs"]) == (o["status"], o["iterations"], o["final_pairs"]), what
            assert np.array_equal(r["idx"], o["idx"]), what
            R = r["T"][:3, :3].astype(np.float64)
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-5 and np.linalg.det(R) > 0, what
            if kind != "collinear":
                assert _T_close(r["T"], o["T"]), (what, r["T"], o["T"])
                continue
            # a collinear cloud does not determine the rotation about its line: compare what it does determine, the
            # image of the (source) line direction under R, and where T takes the source centroid
            d = _rot(0.5, -0.3, 0.4) @ np.array([0.6, 0.0, 0.8])
            oR = o["T"][:3, :3].astype(np.float64)
            assert np.abs(R @ d - oR @ d).max() < 1e-5, (what, R @ d, oR @ d)
            c = np.append(src.astype(np.float64).mean(1), 1.0)
            Tc, oTc = r["T"].astype(np.float64) @ c, o["T"].astype(np.float64) @ c
            assert np.abs(Tc - oTc).max() < 1e-5 * max(1.0, float(np.abs(oTc).max())), (what, Tc, oTc)


@pytest.mark.parametrize("npts", [3, 4])
def test_min_pairs_boundary(ctx, oracle, npts):
    """npts pairs (every point within range): min_pairs <= npts solves, min_pairs = npts + 1 falls back at iteration 0
    (icp.cpp:163-182) with the caller's last motion applied to the working source."""
    rng = np.random.default_rng(40 + npts)
    tgt = (rng.uniform(-1, 1, (3, npts)) + 5).astype(np.float32)
    src = (tgt + np.float32([[0.01], [-0.02], [0.015]])).astype(np.float32)
    lr = _rot(1.0, -2.0, 0.5).astype(np.float32)
    lt = np.float32([0.01, 0.02, -0.03])
    for min_pairs in range(1, 6):
        for solve in (binding.SOLVE_REFERENCE, binding.SOLVE_KABSCH):
            kw = dict(max_iterations=5, threshold=1e-12, min_pairs=min_pairs, solve=solve)
            o = oracle.align(src, tgt, sum_order=1, last_rotation=lr, last_translation=lt, threads=1, **kw)
            runs = [_run(ctx, src, tgt, host_loop=h, last_rotation=lr, last_translation=lt, **kw) for h in (0, 1)]
            what = (npts, min_pairs, solve)
            _assert_same_run(runs[0], runs[1], what)
            r = runs[0]
            if min_pairs <= npts:
                assert o["status"] == binding.OK and o["iterations"] >= 1, what
            else:
                assert o["status"] == binding.W_TOO_FEW_PAIRS and o["iterations"] == 0, what
            assert (r["status"], r["iterations"], r["final_pairs"]) == (o["status"], o["iterations"], o["final_pairs"]), what
            assert np.array_equal(r["idx"], o["idx"]), what
            assert np.array_equal(r["src"].view(np.uint32), o["src_out"].view(np.uint32)), what
            assert _T_close(r["T"], o["T"]), what


@pytest.mark.parametrize("min_pairs", [0, -1])
def test_min_pairs_below_one_is_refused(ctx, oracle, min_pairs):
    """min_pairs < 1 lets a sweep with no pair in range reach the solve, which divides by the zero count: the oracle
    returns status OK with a NaN transform, and the device loop's Kabsch NaN (+NaN) was not the host loop's (-NaN).
    icpk_align (both loops, every NN mode) and icpk_align_batch refuse it with ICPK_E_ARG, and the context is usable
    afterwards; min_pairs = 1 with no pair in range falls back on every path, as the oracle does."""
    p = synth.frustum_pair(500, seed=3)
    src, tgt = p["source"], p["target"]
    far = (src + np.float32(100)).astype(np.float32)
    for solve in (binding.SOLVE_REFERENCE, binding.SOLVE_KABSCH):
        o = oracle.align(far, tgt, max_iterations=3, min_pairs=min_pairs, solve=solve, sum_order=1, fixed_iterations=True,
                         threads=1)
        assert o["status"] == binding.OK and o["final_pairs"] == 0 and np.isnan(o["T"][:3, 3]).all()
        kw = dict(max_iterations=3, fixed_iterations=1, min_pairs=min_pairs, solve=solve)
        for mode in (binding.NN_EXACT, binding.NN_GRID):
            for h in (0, 1):
                ctx.set_target(tgt)
                ctx.set_source(far)
                with pytest.raises(binding.IcpkError) as e:
                    ctx.align(nn_mode=mode, host_loop=h, **kw)
                assert e.value.code == binding.E_ARG
        Tb, stb, rcb = ctx.align_batch([(src, tgt), (far, tgt)], nn_mode=binding.NN_GRID, **kw)
        assert rcb == binding.E_ARG
        ok = dict(kw, min_pairs=1)
        o = oracle.align(far, tgt, max_iterations=3, min_pairs=1, solve=solve, sum_order=1, fixed_iterations=True, threads=1)
        assert o["status"] == binding.W_TOO_FEW_PAIRS and o["iterations"] == 0
        runs = [_run(ctx, far, tgt, host_loop=h, nn_mode=binding.NN_GRID, **ok) for h in (0, 1)]
        _assert_same_run(runs[0], runs[1], (min_pairs, solve))
        r = runs[0]
        assert (r["status"], r["iterations"], r["final_pairs"]) == (o["status"], o["iterations"], 0)
        assert np.array_equal(r["src"].view(np.uint32), o["src_out"].view(np.uint32))
        assert _T_close(r["T"], o["T"])
        Tb, stb, rcb = ctx.align_batch([(src, tgt), (far, tgt)], nn_mode=binding.NN_GRID, **ok)
        assert rcb == binding.W_TOO_FEW_PAIRS and stb[0].status == binding.OK
        assert (stb[1].status, stb[1].iterations) == (binding.W_TOO_FEW_PAIRS, 0)
        assert np.array_equal(Tb[1].view(np.uint32), r["T"].view(np.uint32))


# frozen from a search with the CPU oracle: uniform cloud rotated by up to 20 degrees, reference flavour, 0.1 m range;
# the pair count of the sweep entering iteration K first drops below MIN_PAIRS there
MID_SEED, MID_N, MID_MIN_PAIRS, MID_K, MID_MAX_NN = 62, 150, 13, 2, 0.1
MID_LR, MID_LT = (1.0, 2.0, 3.0), (0.01, 0.02, -0.03)


def _mid_pair():
    from oracle import icp_oracle

    rng = np.random.default_rng(MID_SEED)
    n = int(rng.integers(30, 300))
    assert n == MID_N
    tgt = rng.uniform(-1, 1, (3, n)).astype(np.float32)
    ang = rng.uniform(-20, 20, 3)
    R = icp_oracle.make_rotation_matrix(*ang).astype(np.float64)
    src = (R @ tgt + rng.normal(0, 0.1, (3, 1)) + rng.normal(0, 0.01, (3, n))).astype(np.float32)
    return src, tgt


def _mid_kw():
    from oracle import icp_oracle

    return dict(max_iterations=16, threshold=1e-9, max_nn_dist=MID_MAX_NN, min_pairs=MID_MIN_PAIRS,
                solve=binding.SOLVE_REFERENCE, last_rotation=icp_oracle.make_rotation_matrix(*MID_LR),
                last_translation=np.float32(MID_LT))


def test_mid_loop_fallback_every_loop_ahead(oracle, monkeypatch):
    """The fallback at iteration MID_K >= 2 of a threshold-mode loop: status W_TOO_FEW_PAIRS, MID_K iterations and
    trace entries, the caller's last motion applied to the working source (get_source() == the oracle's src_out bit for
    bit), T within 1e-5 of the oracle's; identical for every ICPK_LOOP_AHEAD and both loops."""
    src, tgt = _mid_pair()
    kw = _mid_kw()
    o = oracle.align(src, tgt, sum_order=1, threads=1, **kw)
    assert o["status"] == binding.W_TOO_FEW_PAIRS and o["iterations"] == MID_K >= 2
    assert all(t["n_pairs"] >= MID_MIN_PAIRS for t in o["trace"]) and o["final_pairs"] < MID_MIN_PAIRS
    first = None
    for ahead in (0, 1, 2, 6):
        monkeypatch.setenv("ICPK_LOOP_AHEAD", str(ahead))
        with binding.Context(0) as c:
            for h in (0, 1):
                r = _run(c, src, tgt, host_loop=h, **kw)
                what = (ahead, h)
                assert r["rc"] == r["status"] == binding.W_TOO_FEW_PAIRS and r["iterations"] == MID_K, what
                assert len(r["trace"]) == MID_K and r["final_pairs"] == o["final_pairs"], what
                assert np.array_equal(r["src"].view(np.uint32), o["src_out"].view(np.uint32)), what
                assert np.array_equal(r["idx"], o["idx"]), what
                assert _T_close(r["T"], o["T"]), what
                if first is None:
                    first = r
                else:
                    _assert_same_run(first, r, what)


def test_mid_loop_fallback_inside_a_frame_batch(ctx):
    """The same pair in slot 1 of a frame batch, between pairs that converge normally: its slot gives the single call's
    results."""
    src, tgt = _mid_pair()
    kw = _mid_kw()
    single = _run(ctx, src, tgt, **kw)
    pairs = []
    for seed in (31, 32):
        q = synth.frustum_pair(800, seed=seed, rot_deg=(0.3, -0.2, 0.4), shift=(0.01, 0.0, -0.005))
        pairs.append((q["source"], q["target"]))
    pairs.insert(1, (src, tgt))
    alone = [_run(ctx, s, t, **kw) for s, t in pairs]
    Tb, stb, rcb, assoc = ctx.align_batch(pairs, associations=True, **kw)
    assert alone[1]["status"] == binding.W_TOO_FEW_PAIRS and alone[0]["status"] == alone[2]["status"] == binding.OK
    for b, r in enumerate(alone):
        assert (stb[b].status, stb[b].iterations, stb[b].final_pairs) == (r["status"], r["iterations"], r["final_pairs"]), b
        assert np.array_equal(Tb[b].view(np.uint32), r["T"].view(np.uint32)), b
        assert np.array_equal(assoc[b][0], r["idx"]), b
    assert np.array_equal(single["T"].view(np.uint32), Tb[1].view(np.uint32))
