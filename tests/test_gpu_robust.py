"""Robust alignment on the device (include/icpk.h, icpk_set_robust) against the float64 model
(tests/robust_model.py), the plain flavours and itself (device loop == host loop)."""
import functools
import itertools
import math

import numpy as np
import pytest

import robust_model as rm
from icp_slam_prototype_amd import binding, synth

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
TUKEY_MEDIAN_08 = dict(kernel=rm.TUKEY, scale=4.685, scale_mode=rm.MEDIAN, trim=0.8)
HUBER_MEDIAN = dict(kernel=rm.HUBER, scale=1.0, scale_mode=rm.MEDIAN, trim=1.0)
QUALITY = dict(rot=1e-4, trans=1e-4)  # tests/test_robust_host.py: the model's bounds on the contaminated pair


@pytest.fixture(scope="module")
def ctx():
    from icp_slam_prototype_amd import build

    build.build()
    c = binding.Context(0)
    yield c
    c.close()


def set_robust(ctx, cfg):
    if cfg is None:
        ctx.set_robust(None)
    else:
        ctx.set_robust(kernel=cfg["kernel"], scale=cfg["scale"], scale_mode=cfg["scale_mode"], trim=cfg["trim"])


def cloud(n, seed, nt=3000):
    rng = np.random.default_rng(seed)
    tgt = (rng.uniform(-2, 2, (3, nt)) + 5).astype(np.float32)
    src = (tgt[:, rng.integers(0, nt, n)] + rng.normal(0, 0.03, (3, n))).astype(np.float32)
    return src, tgt


def check_reduce_weighted(ctx, src, tgt, cfg, max_dist, tn=None):
    """icpk_reduce_weighted against the model: tau, m, c bit-exact, counts exact, sums within the tree's bound.
    tn: the target's normals, for the point-to-plane flavour (K5's 30 sums) in place of Kabsch's 21"""
    set_robust(ctx, cfg)
    ctx.set_target(tgt)
    if tn is not None:
        ctx.set_target_normals(tn)
    ctx.set_source(src)
    idx, dist = ctx.nn(binding.NN_EXACT)
    if tn is None:
        sums, n, kept, cut, med, c = ctx.reduce_weighted(max_dist)
        acc, w, tau, m, mc = rm.robust_weights(dist, max_dist, cfg)
    else:
        sums, n, kept, cut, med, c = ctx.reduce_weighted(max_dist, solve=binding.SOLVE_POINT_TO_PLANE)
        acc, w, tau, m, mc = rm.robust_weights(dist, max_dist, cfg, idx, tn)
    assert n == np.count_nonzero(acc)
    assert kept == np.count_nonzero(w > 0)
    assert cut.view(np.uint32) == np.float32(tau).view(np.uint32) and med.view(np.uint32) == np.float32(m).view(np.uint32)
    assert c == mc
    # the kernel's terms, evaluated in the same order in numpy: bit-identical terms, so only the tree's rounding is left
    a = src[:, acc].astype(np.float64)
    b = tgt[:, idx[acc]].astype(np.float64)
    ww = w[acc]
    k = ww > 0
    if tn is None:
        wb = [ww * b[r] for r in range(3)]
        terms = [(wb[r] * a[cc])[k] for r in range(3) for cc in range(3)]
        terms += [(ww * (src[cc, acc] - tgt[cc, idx[acc]]).astype(np.float64))[k] for cc in range(3)]
        terms += [dist[acc].astype(np.float64)]
        terms += [(ww * a[cc])[k] for cc in range(3)] + [wb[cc][k] for cc in range(3)]
    else:
        nr = tn[:, idx[acc]].astype(np.float64)
        J = [a[1] * nr[2] - a[2] * nr[1], a[2] * nr[0] - a[0] * nr[2], a[0] * nr[1] - a[1] * nr[0], nr[0], nr[1], nr[2]]
        r = ((a[0] - b[0]) * nr[0] + (a[1] - b[1]) * nr[1]) + (a[2] - b[2]) * nr[2]
        terms = [(ww * (J[i] * J[j]))[k] for i in range(6) for j in range(i, 6)]
        terms += [(ww * (J[i] * r))[k] for i in range(6)]
        terms += [dist[acc].astype(np.float64)]
    terms += [ww[k], np.ones(int(k.sum()))]
    nb = min(max((len(dist) + 255) // 256, 1), 256)
    chain = -(-len(dist) // (256 * nb)) + 18
    for s, t in enumerate(terms):
        exact = math.fsum(t.tolist())
        assert abs(sums[s] - exact) <= chain * U * float(np.sum(np.abs(t))), (len(dist), s, sums[s], exact)
    assert len(sums) == len(terms) and sums[-1] == kept


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537, 92000, 1_000_003])
def test_reduce_weighted_against_model(ctx, n):
    """both flavours (the point-to-plane one with unit normals and, every fifth, none) at one pair, on each side of a
    block, and beyond 65536 pairs, where a lane takes more than one"""
    src, tgt = cloud(n, seed=n)
    if n >= 255:
        src[:, n // 3] = np.nan  # never accepted
    tn = np.random.default_rng(n).normal(size=tgt.shape)
    tn = (tn / np.linalg.norm(tn, axis=0)).astype(np.float32)
    tn[:, 2::5] = 0  # never accepted
    for cfg in (TUKEY_MEDIAN_08, HUBER_MEDIAN, dict(kernel=rm.TUKEY, scale=0.05, scale_mode=rm.FIXED, trim=0.5)):
        check_reduce_weighted(ctx, src, tgt, cfg, 0.75)
        if n < 1_000_000:  # (the model of a million pairs once is enough)
            check_reduce_weighted(ctx, src, tgt, cfg, 0.75, tn)


def test_reduce_weighted_ties_zeros_and_gate(ctx):
    p = synth.lattice_wall()  # many equal distances: the cut falls inside a run of ties
    check_reduce_weighted(ctx, p["source"], p["target"], TUKEY_MEDIAN_08, 0.75)
    check_reduce_weighted(ctx, p["source"], p["target"], dict(rm.IDENTITY, trim=0.3), 0.75)
    tgt = cloud(10, 3, nt=5000)[1]
    check_reduce_weighted(ctx, tgt.copy(), tgt, TUKEY_MEDIAN_08, 0.75)  # every distance 0: tau = m = c = 0, w = 1
    sums, n, kept, cut, med, c = ctx.reduce_weighted(0.75)
    assert n == kept == 5000 and cut == 0 and med == 0 and c == 0.0
    src, tgt = cloud(20000, 9)
    ctx.set_target(tgt)
    ctx.set_source(src)
    _, dist = ctx.nn(binding.NN_EXACT)
    edge = float(np.sort(dist)[15000])  # a distance that occurs: pairs exactly on max_dist are not accepted
    check_reduce_weighted(ctx, src, tgt, HUBER_MEDIAN, edge)
    # nothing accepted: zero sums, counts and selection
    set_robust(ctx, HUBER_MEDIAN)
    sums, n, kept, cut, med, c = ctx.reduce_weighted(0.0)
    assert n == kept == 0 and not sums.any() and cut == med == 0


def test_reduce_weighted_p2l_selection(ctx, oracle):
    fx, cx = float(synth.K2_FX) / 2, float(synth.K2_CX) / 2
    p = synth.kinect_pair(rows=212, cols=256, valid=1.0, seed=8, fx=fx, cx=cx)
    pts, nrm = oracle.backproject_normals(p["depth_tgt"], 0, fx=fx, cx=cx)
    ctx.backproject_with_normals(p["depth_tgt"], 0, fx=fx, cx=cx, offset=[5, 5, 5])
    ctx.set_source(p["source"])
    set_robust(ctx, TUKEY_MEDIAN_08)
    idx, dist = ctx.nn()
    sums, n, kept, cut, med, c = ctx.reduce_weighted(0.3, solve=binding.SOLVE_POINT_TO_PLANE)
    acc, w, tau, m, mc = rm.robust_weights(dist, 0.3, TUKEY_MEDIAN_08, idx, nrm)
    assert n == np.count_nonzero(acc) > 1000 and kept == np.count_nonzero(w > 0) == sums[29]
    assert cut == tau and med == m and c == mc
    assert abs(sums[28] - math.fsum(w.tolist())) <= 1e-12 * n
    assert abs(sums[27] - math.fsum(dist[acc].astype(np.float64).tolist())) <= 1e-12 * sums[27]


def kinect_small(seed=3):
    return synth.kinect_pair(rows=120, cols=160, valid=0.6, seed=seed)


@functools.lru_cache(maxsize=None)
def kinect_big():
    """more than 65536 points: a lane of the reduction takes several pairs"""
    return synth.kinect_pair(rows=240, cols=320, valid=0.9, seed=5, fx=synth.FX / 2, cx=synth.CX / 2)


def load_pair(ctx, p, p2l):
    if p2l:
        ctx.backproject_with_normals(p["depth_tgt"], 0, fx=p["fx"], cx=p["cx"], offset=[0, 0, 0])
        ctx.backproject(p["depth_src"], which=0, fx=p["fx"], cx=p["cx"], offset=[0, 0, 0])
    else:
        ctx.set_target(p["target"])
        ctx.set_source(p["source"])


def run(ctx, cfg, **kw):
    set_robust(ctx, cfg)
    T, st, rc = ctx.align(**kw)
    return (T, (st.iterations, st.status, st.final_pairs, np.float32(st.final_mse).view(np.uint32), st.nn_launches),
            ctx.get_trace(), ctx.get_robust_trace(), rc)


def same(a, b, robust_trace=True):
    Ta, sa, tra, rta, rca = a
    Tb, sb, trb, rtb, rcb = b
    assert rca == rcb and sa == sb
    assert np.array_equal(Ta.view(np.uint32), Tb.view(np.uint32))
    assert len(tra) == len(trb)
    for x, y in zip(tra, trb):
        assert np.array_equal(x["R"].view(np.uint32), y["R"].view(np.uint32))
        assert np.array_equal(x["t"].view(np.uint32), y["t"].view(np.uint32))
        assert x["n_pairs"] == y["n_pairs"] and x["mse"].view(np.uint32) == y["mse"].view(np.uint32)
    if robust_trace:
        assert rta == rtb


@pytest.mark.parametrize("solve,nn_mode,host_loop", list(itertools.product(
    [binding.SOLVE_KABSCH, binding.SOLVE_POINT_TO_PLANE], [binding.NN_GRID, binding.NN_EXACT], [0, 1])))
def test_identity_setting_equals_plain(ctx, solve, nn_mode, host_loop):
    p2l = solve == binding.SOLVE_POINT_TO_PLANE
    load_pair(ctx, kinect_small(), p2l)
    kw = dict(solve=solve, nn_mode=nn_mode, host_loop=host_loop, max_iterations=8, fixed_iterations=1,
              max_nn_dist=0.3 if p2l else 0.75)
    plain = run(ctx, None, **kw)
    assert plain[3] == []  # no robust record after a plain alignment
    ident = run(ctx, dict(rm.IDENTITY, scale=0.37), **kw)
    same(plain, ident, robust_trace=False)
    for tr, rt in zip(ident[2], ident[3]):
        assert rt["kept"] == tr["n_pairs"] and rt["wsum"] == float(tr["n_pairs"]) and rt["c"] == float(np.float32(0.37))


@pytest.mark.parametrize("kernel,scale_mode,trim", list(itertools.product([rm.NONE, rm.HUBER, rm.TUKEY],
                                                                           [rm.FIXED, rm.MEDIAN], [1.0, 0.8])))
def test_device_loop_equals_host_loop(ctx, kernel, scale_mode, trim):
    scale = {rm.NONE: 1.0, rm.HUBER: 1.0 if scale_mode == rm.MEDIAN else 0.02,
             rm.TUKEY: 4.685 if scale_mode == rm.MEDIAN else 0.1}[kernel]
    cfg = dict(kernel=kernel, scale=scale, scale_mode=scale_mode, trim=trim)
    for p2l, fixed in itertools.product((False, True), (1, 0)):
        load_pair(ctx, kinect_small(seed=5), p2l)
        kw = dict(solve=binding.SOLVE_POINT_TO_PLANE if p2l else binding.SOLVE_KABSCH, max_iterations=12,
                  fixed_iterations=fixed, threshold=1e-7, max_nn_dist=0.3 if p2l else 0.75)
        dev = run(ctx, cfg, host_loop=0, **kw)
        host = run(ctx, cfg, host_loop=1, **kw)
        same(dev, host)
        assert len(dev[3]) == dev[1][0] > 0
    for p2l in (False, True):
        load_pair(ctx, kinect_big(), p2l)
        assert ctx.get_source().shape[1] > 65536
        kw = dict(solve=binding.SOLVE_POINT_TO_PLANE if p2l else binding.SOLVE_KABSCH, max_iterations=4,
                  fixed_iterations=1, max_nn_dist=0.3 if p2l else 0.75)
        dev = run(ctx, cfg, host_loop=0, **kw)
        same(dev, run(ctx, cfg, host_loop=1, **kw))
        assert len(dev[3]) == dev[1][0] == 4


@pytest.mark.parametrize("which", ["contaminated", "kinect"])
def test_loop_matches_model(ctx, oracle, which):
    p = rm.contaminated_pair() if which == "contaminated" else synth.kinect_pair()
    load_pair(ctx, p, False)
    T, st, tr, rt, rc = run(ctx, HUBER_MEDIAN, solve=binding.SOLVE_KABSCH, max_iterations=20, fixed_iterations=1)
    To, kept, cuts, sto = rm.align(p["source"], p["target"], oracle, HUBER_MEDIAN, iterations=20)
    assert rc == sto == 0 and st[0] == 20
    assert [e["kept"] for e in rt] == kept
    assert np.abs(T.astype(np.float64) - To).max() < 1e-5


def test_contaminated_quality_on_device(ctx):
    p = rm.contaminated_pair()
    load_pair(ctx, p, False)
    T0 = run(ctx, None, solve=binding.SOLVE_KABSCH, max_iterations=20, fixed_iterations=1)[0]
    T1 = run(ctx, HUBER_MEDIAN, solve=binding.SOLVE_KABSCH, max_iterations=20, fixed_iterations=1)[0]
    r0, t0 = rm.motion_error(T0.astype(np.float64), p)
    r1, t1 = rm.motion_error(T1.astype(np.float64), p)
    assert r1 < QUALITY["rot"] and t1 < QUALITY["trans"], (r1, t1)
    assert not (r0 < QUALITY["rot"] and t0 < QUALITY["trans"]), (r0, t0)


def test_too_few_kept_pairs_fall_back(ctx):
    lastR = synth.rot_xyz_deg(0, 1, 0).astype(np.float32)
    lastT = np.float32([0.01, 0, 0])
    p = rm.contaminated_pair()
    # first sweep: a Tukey scale far below every distance keeps nothing
    load_pair(ctx, p, False)
    kw = dict(solve=binding.SOLVE_KABSCH, max_iterations=10, fixed_iterations=1, last_rotation=lastR,
              last_translation=lastT)
    tiny = dict(kernel=rm.TUKEY, scale=1e-7, scale_mode=rm.FIXED, trim=1.0)
    dev, host = run(ctx, tiny, host_loop=0, **kw), run(ctx, tiny, host_loop=1, **kw)
    same(dev, host)
    assert dev[4] == binding.W_TOO_FEW_PAIRS and dev[1][0] == 0 and dev[1][2] == 10000
    assert np.array_equal(dev[0], np.eye(4, dtype=np.float32))
    moved = ctx.get_source()
    ref = binding.Context(0)
    try:  # the fallback applied the caller's last motion to the source, as the plain path's fallback does
        ref.set_target(p["target"])
        ref.set_source(p["source"])
        ref.transform_source(lastR, lastT)
        assert np.array_equal(moved, ref.get_source())
    finally:
        ref.close()
    # mid-loop: the median-scaled Tukey keeps fewer pairs as the loop converges; a min_pairs between the first and
    # the last kept count stops it part way
    cfg = dict(kernel=rm.TUKEY, scale=4.685, scale_mode=rm.MEDIAN, trim=1.0)
    kept = [e["kept"] for e in run(ctx, cfg, solve=binding.SOLVE_KABSCH, max_iterations=10, fixed_iterations=1)[3]]
    assert kept[0] > min(kept[1:])
    mp = (kept[0] + min(kept[1:])) // 2 + 1
    stop = next(i for i, k in enumerate(kept) if k < mp)
    dev, host = run(ctx, cfg, host_loop=0, min_pairs=mp, **kw), run(ctx, cfg, host_loop=1, min_pairs=mp, **kw)
    same(dev, host)
    assert dev[4] == binding.W_TOO_FEW_PAIRS and dev[1][0] == stop > 0


def test_degenerate_step_leaves_no_robust_trace_entry(ctx):
    """Found by soak_cases.soak_flavours("robust_p2l", seed 32074: a plane, one normal everywhere): the 6 x 6 system is
    singular at the first step.  That iteration is not completed, so it has no entry in the trace or in the robust
    trace; the host loop used to leave a robust entry for it, the device loop none."""
    w = synth.lattice_wall(rows=30, cols=40)
    tn = np.tile(np.float32([[0], [0], [-1]]), (1, w["target"].shape[1]))
    try:
        for cfg in (HUBER_MEDIAN, TUKEY_MEDIAN_08, dict(rm.IDENTITY, trim=0.5)):
            runs = []
            for nn_mode, host_loop in ((binding.NN_GRID, 0), (binding.NN_EXACT, 1), (binding.NN_GRID, 1)):
                ctx.set_target(w["target"])
                ctx.set_target_normals(tn)
                ctx.set_source(w["source"])
                runs.append(run(ctx, cfg, solve=binding.SOLVE_POINT_TO_PLANE, nn_mode=nn_mode, host_loop=host_loop,
                                max_iterations=5, fixed_iterations=1))
            for r in runs:
                assert r[4] == binding.W_DEGENERATE and r[1][:2] == (0, binding.W_DEGENERATE) and r[1][2] > 1000
                assert r[2] == [] and r[3] == []
                assert r[0].tobytes() == runs[0][0].tobytes() and r[1][:4] == runs[0][1][:4]
    finally:
        set_robust(ctx, None)


def test_refusals_and_reset(ctx):
    p = kinect_small(seed=7)
    load_pair(ctx, p, False)
    plain = run(ctx, None, solve=binding.SOLVE_KABSCH, max_iterations=6, fixed_iterations=1)
    set_robust(ctx, HUBER_MEDIAN)
    with pytest.raises(binding.IcpkError) as e:
        ctx.align(solve=binding.SOLVE_REFERENCE)
    assert e.value.code == binding.E_ARG
    job = dict(stream=0, source=p["depth_src"], target=p["depth_tgt"])
    _, _, rc = ctx.align_frames_batch([job], solve=binding.SOLVE_KABSCH)
    assert rc == binding.E_ARG
    for bad in (dict(kernel=3), dict(kernel=-1), dict(scale_mode=2), dict(scale=0.0), dict(scale=-1.0),
                dict(scale=float("inf")), dict(scale=float("nan")), dict(trim=0.0), dict(trim=1.5),
                dict(trim=float("nan"))):
        with pytest.raises(binding.IcpkError) as e:
            set_robust(ctx, dict(HUBER_MEDIAN, **bad))
        assert e.value.code == binding.E_ARG
    robust = run(ctx, HUBER_MEDIAN, solve=binding.SOLVE_KABSCH, max_iterations=6, fixed_iterations=1)
    assert not np.array_equal(robust[0], plain[0])
    same(run(ctx, None, solve=binding.SOLVE_KABSCH, max_iterations=6, fixed_iterations=1), plain)
    # align_batch with robust on: the pairs one by one, each equal to icpk_align
    pairs = [(q["source"], q["target"]) for q in (kinect_small(seed=s) for s in (11, 12, 13))]
    set_robust(ctx, TUKEY_MEDIAN_08)
    Tb, stb, rcb = ctx.align_batch(pairs, solve=binding.SOLVE_KABSCH, max_iterations=6, fixed_iterations=1)
    assert rcb == 0
    for b, (s, t) in enumerate(pairs):
        ctx.set_target(t)
        ctx.set_source(s)
        T, st, rc = ctx.align(solve=binding.SOLVE_KABSCH, max_iterations=6, fixed_iterations=1)
        assert np.array_equal(Tb[b].view(np.uint32), T.view(np.uint32)) and stb[b].final_pairs == st.final_pairs


def test_align_to_map_honours_robust(ctx):
    p = kinect_small(seed=21)
    set_robust(ctx, TUKEY_MEDIAN_08)
    ctx.map_reset()
    ctx.map_update_points(binding.MAP_ADD_CLOUD, p["target"], 180)
    keys = np.stack(ctx.map_get_list(binding.MAP_KEYPOINTS))
    assert keys.shape[1] > 100
    ctx.set_source(p["source"])
    kw = dict(solve=binding.SOLVE_KABSCH, max_iterations=6, fixed_iterations=1, max_nn_dist=0.1)
    T, st, rc = ctx.align_to_map(delta=25, **kw)
    rt = ctx.get_robust_trace()
    ref = binding.Context(0)
    try:
        set_robust(ref, TUKEY_MEDIAN_08)
        ref.set_target(keys)
        ref.set_source(p["source"])
        Tr, sr, rcr = ref.align(**kw)
        assert rc == rcr and st.iterations == sr.iterations and st.final_pairs == sr.final_pairs
        assert np.array_equal(T.view(np.uint32), Tr.view(np.uint32))
        assert rt == ref.get_robust_trace() and len(rt) == st.iterations
    finally:
        ref.close()
    ctx.map_release()
