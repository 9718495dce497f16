"""Pose-graph optimisation on the device (K18) against the CPU model of tests/posegraph_model.py: one evaluation, the
optimum of the shared cases, the same bytes on every run, the shapes at which the kernels take another path, what the
call leaves alone, and a graph made from clouds.

The tolerance of the comparing tests is 16 x s_graph, the graph's sensitivity to the order of a node's gather.  A node
with two incident edges sums a + b = b + a exactly, so on a ring or a chain s_graph is 0 (case A, two_nodes, chain_257,
reference_last) and the bound asks for the model's bytes.  The rule is written without libm and the model restates it
operation for operation, so that is what the device gives.  The star's hub is a FREE node (the reference node is a
leaf), so its gather of 64 edges feeds the solve and the step, and its gradient is held against the model too.

MEASURED on an MI355X: see DESIGN.md K18, "Measured / unmeasured on the device"."""
import numpy as np
import pytest

import posegraph_cases as pc
import posegraph_model as pm
from icp_slam_prototype_amd import binding
from icp_slam_prototype_amd.posegraph import PoseGraph

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def ctx():
    with binding.Context(0) as c:
        yield c


# ---- evaluate --------------------------------------------------------------------------------------------------------
def _evaluate_bounds(poses, edges, mu):
    """Bounds that follow from float64 and the number of terms.  An entry of the residual r comes out of three products
    of 3 terms each over entries up to `scale` and the rotation vector: about 32 roundings of numbers up to scale, so
    |dr| <= 32 eps scale.  The kernel takes the rotation's angle as atan2(|v|, (trace - 1) / 2) (not acos of the trace,
    which would lose half the digits at small angles): its relative error is a few eps and is inside the 32.  chi2 = r^T
    L r moves by 2 |L| |r| dr, plus 16 eps chi2 for its own 42 terms; l by |dl / dchi2| <= 2 / mu of that; the cost by
    the sum of its terms' bounds plus one eps per level of its tree; a node's gradient by the sum over its edges of
    |J^T| |l L| dr (the residual's share) + 64 eps |J^T| |l L| |r| (J's own entries and the 72 terms of the products)."""
    n = len(poses)
    scale = max(1.0, float(np.abs(poses).max()), max(float(np.abs(ed[2]).max()) for ed in edges))
    dr = 32 * EPS * scale
    chi2, l, cost, _ = pm.evaluate(poses, edges, mu)
    tol_chi2, tol_g = np.zeros(len(edges)), np.zeros((n, 6))
    for e, (s, t, T, info, unc) in enumerate(edges):
        r, tB = pm.residual(poses[s], poses[t], T)
        tol_chi2[e] = 2 * dr * float(np.sum(np.abs(info) @ np.abs(r))) + 6 * dr * dr * float(np.abs(info).sum()) + 16 * EPS * chi2[e]
        J = np.abs(pm.jacobian_source(poses[t], r, tB))
        tg = J.T @ (l[e] * np.abs(info)) @ (dr * np.ones(6) + 64 * EPS * scale * np.abs(r))
        tol_g[s] += tg
        tol_g[t] += tg
    tol_l = (2 * tol_chi2 / mu if mu > 0 else 0.0) + 4 * EPS
    tol_cost = float(tol_chi2.sum()) + 16 * EPS * cost
    return tol_chi2, tol_l, tol_cost, tol_g


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_evaluate_equals_the_model(ctx, name):
    c = pc.case(name)
    mu = c["params"].get("preference_loop_closure", 0.0)
    chi2, l, cost, g = ctx.pose_graph_evaluate(c["poses"], c["edges"], mu)
    mchi2, ml, mcost, mg = pm.evaluate(c["poses"], c["edges"], mu)
    tol_chi2, tol_l, tol_cost, tol_g = _evaluate_bounds(c["poses"], c["edges"], mu)
    print(f"case {name}: evaluate vs model: chi2 {np.abs(chi2 - mchi2).max():.3e} (bound {tol_chi2.max():.3e}), "
          f"l {np.abs(l - ml).max():.3e}, cost {abs(cost - mcost):.3e} (bound {tol_cost:.3e}), "
          f"gradient {np.abs(g - mg).max():.3e} (bound {tol_g.max():.3e})")
    assert np.all(np.abs(chi2 - mchi2) <= tol_chi2)
    assert np.all(np.abs(l - ml) <= tol_l)
    assert abs(cost - mcost) <= tol_cost
    assert np.all(np.abs(g - mg) <= tol_g)
    if name == "C":
        assert l[-1] < 1.0 and np.all(l[:15] == 1.0)


# ---- optimize --------------------------------------------------------------------------------------------------------
def _compare(tag, got, res, want, s_graph):
    """the device's poses and cost within 16 x the graph's sensitivity to summation order of the model's"""
    dp = float(np.abs(got - want["poses"]).max())
    dc = abs(res.final_cost - want["final_cost"]) / max(want["final_cost"], np.finfo(float).tiny)
    print(f"{tag}: device vs model: pose {dp:.3e}, relative cost {dc:.3e}, s_graph {s_graph:.3e}, bound {16 * s_graph:.3e}; "
          f"iterations {res.iterations} / {want['iterations']}, accepted {res.accepted} / {want['accepted']}, "
          f"pcg {res.pcg_iterations} / {want['pcg_iterations']}")
    assert dp <= 16 * s_graph
    assert dc <= 16 * s_graph


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_optimum_equals_the_model(ctx, name):
    c = pc.case(name)
    want = pc.model_result(name)
    P, res, w, chi2, pruned, rc = ctx.pose_graph_optimize(c["poses"], c["edges"], **pc.binding_params(c["params"]))
    trace = ctx.get_pose_graph_trace()
    pattern = [t["accepted"] for t in trace]
    print(f"case {name}: accepted pattern equal to the model's: {pattern == [t['accepted'] for t in want['trace']]}; "
          f"error against the truth {pc.pose_error(c['poses'], c['truth']):.4f} -> {pc.pose_error(P, c['truth']):.4f}")
    assert rc == binding.OK and len(trace) == res.iterations
    assert P[0].tobytes() == np.ascontiguousarray(c["poses"][0]).tobytes()
    assert res.final_cost < res.initial_cost
    if name == "C":
        e = [k for k, ed in enumerate(c["edges"]) if (ed[0], ed[1]) == pc.FALSE_CLOSURE]
        assert list(np.nonzero(pruned)[0]) == e and res.n_pruned == 1
        assert w[e[0]] < 0.25 and np.all(w[15:17] > 0.99)
    else:
        assert not pruned.any() and np.all(w == 1.0)
    _compare(f"case {name}", P, res, want, pc.s_graph(name))


def test_same_bytes_on_every_call_and_context(ctx):
    c = pc.case("C")
    kw = pc.binding_params(c["params"])
    runs = []
    for k in range(3):
        P, res, w, chi2, pruned, rc = ctx.pose_graph_optimize(c["poses"], c["edges"], **kw)
        runs.append((P.tobytes(), w.tobytes(), chi2.tobytes(), repr(ctx.get_pose_graph_trace())))
    with binding.Context(0) as other:
        P, res, w, chi2, pruned, rc = other.pose_graph_optimize(c["poses"], c["edges"], **kw)
        runs.append((P.tobytes(), w.tobytes(), chi2.tobytes(), repr(other.get_pose_graph_trace())))
    assert all(r == runs[0] for r in runs[1:])


def test_nothing_to_do(ctx):
    truth = pc.ring_poses(12)
    pairs = [(i + 1, i) for i in range(11)] + [(11, 0), (6, 1)]
    rng = np.random.default_rng(3)
    edges = [(s, t, pm.inv_pose(truth[t]) @ truth[s], pc.information(rng), False) for s, t in pairs]
    P, res, w, chi2, pruned, rc = ctx.pose_graph_optimize(truth, edges)
    trace = ctx.get_pose_graph_trace()
    print(f"nothing to do: initial cost {res.initial_cost:.3e}, iterations {res.iterations}, moved {np.abs(P - truth).max():.3e}")
    assert rc == binding.OK
    assert res.initial_cost < 1e-20 * len(edges)
    assert res.iterations <= 1 and len(trace) == res.iterations
    assert np.abs(P - truth).max() <= 10 * 1e-10  # no step larger than step_tolerance (on poses of size <= 4: |dP| <= |P| |d|)


# ---- shapes that can go wrong ----------------------------------------------------------------------------------------
def _shape(name):
    if name == "two_nodes":
        return pc.graph(2, [(1, 0)], 11), dict(max_iterations=10)
    if name == "star_65":  # node 0 has 64 incident edges: its gather is longer than a wave.  It is a free node (the
        # reference node is leaf 1), so H p, the damped block and the step of the hub all come out of that gather
        return pc.graph(65, [(i, 0) for i in range(1, 65)], 12), dict(max_iterations=4, max_pcg_iterations=40, reference_node=1)
    if name == "chain_257":  # past one workgroup of the reduction tree and of the node pass
        return pc.graph(257, [(i + 1, i) for i in range(256)], 13), dict(max_iterations=2, max_pcg_iterations=25)
    if name == "reference_last":
        return pc.graph(9, [(i + 1, i) for i in range(8)] + [(8, 0)], 14), dict(max_iterations=10, reference_node=8)
    if name == "double_edge":
        return pc.graph(6, [(1, 0), (2, 1), (2, 1), (3, 2), (4, 3), (5, 4), (5, 0)], 15), dict(max_iterations=10)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["two_nodes", "star_65", "chain_257", "reference_last", "double_edge"])
def test_shapes(ctx, name):
    g, kw = _shape(name)
    want = pm.optimize(g["poses"], g["edges"], **kw)
    rev = pm.optimize(g["poses"], g["edges"], reverse=True, **kw)
    s_graph = float(np.abs(want["poses"] - rev["poses"]).max())
    P, res, w, chi2, pruned, rc = ctx.pose_graph_optimize(g["poses"], g["edges"], **kw)
    ref = kw.get("reference_node", 0)
    assert rc in (binding.OK, binding.W_NOT_CONVERGED) and (rc == binding.OK) == want["converged"]
    assert P[ref].tobytes() == np.ascontiguousarray(g["poses"][ref]).tobytes()
    assert res.final_cost < res.initial_cost
    _compare(name, P, res, want, s_graph)


def test_star_hub_gradient_equals_the_model(ctx):
    """evaluate leaves no node out: the hub's gradient is its 64-term gather, held against the model within the bounds of
    test_evaluate_equals_the_model"""
    g, _ = _shape("star_65")
    chi2, l, cost, grad = ctx.pose_graph_evaluate(g["poses"], g["edges"])
    mchi2, ml, mcost, mg = pm.evaluate(g["poses"], g["edges"])
    tol_chi2, tol_l, tol_cost, tol_g = _evaluate_bounds(g["poses"], g["edges"], 0.0)
    print(f"star_65 evaluate: hub gradient {np.abs(grad[0] - mg[0]).max():.3e} (bound {tol_g[0].max():.3e}, |g| {np.abs(mg[0]).max():.3e}), "
          f"other nodes {np.abs(grad[1:] - mg[1:]).max():.3e}, cost {abs(cost - mcost):.3e} (bound {tol_cost:.3e})")
    assert np.abs(mg[0]).max() > 1e3 * tol_g[0].max()  # (the hub's gradient is there to be got wrong)
    assert np.all(np.abs(chi2 - mchi2) <= tol_chi2) and np.all(l == 1.0)
    assert abs(cost - mcost) <= tol_cost
    assert np.all(np.abs(grad - mg) <= tol_g)


def test_prune_that_would_cut_a_node_off_prunes_nothing(ctx):
    """the rule's last sentence on pruning, on the device as in the model"""
    g, mkw = pc.prune_bridge_graph()
    want = pm.optimize(g["poses"], g["edges"], **mkw)
    rev = pm.optimize(g["poses"], g["edges"], reverse=True, **mkw)
    s_graph = float(np.abs(want["poses"] - rev["poses"]).max())
    P, res, w, chi2, pruned, rc = ctx.pose_graph_optimize(g["poses"], g["edges"], **pc.binding_params(mkw))
    assert rc == binding.OK and not pruned.any() and res.n_pruned == 0
    assert len(ctx.get_pose_graph_trace()) == res.iterations == want["iterations"]  # (no second run)
    _compare("prune bridge", P, res, want, s_graph)


def test_a_live_context_refuses_a_bad_graph(ctx):
    """the device calls make icpk_pose_graph_check's refusals themselves, and write nothing when they do"""
    c = pc.case("A")
    s, t, T, info, u = c["edges"][2]
    bad = [(c["poses"], c["edges"][:2] + [(t, t, T, info, u)] + c["edges"][3:]),  # s == t
           (c["poses"], c["edges"][:3] + c["edges"][4:7]),                         # nodes 4 .. 7 cut off
           (np.where(np.arange(8)[:, None, None] == 5, np.nan, c["poses"]), c["edges"])]
    for P, E in bad:
        with pytest.raises(binding.IcpkError) as err:
            ctx.pose_graph_optimize(P, E)
        assert err.value.code == binding.E_ARG
        with pytest.raises(binding.IcpkError) as err:
            ctx.pose_graph_evaluate(P, E)
        assert err.value.code == binding.E_ARG
    with pytest.raises(binding.IcpkError) as err:
        ctx.pose_graph_optimize(c["poses"], c["edges"], reference_node=8)
    assert err.value.code == binding.E_ARG
    assert ctx.pose_graph_optimize(c["poses"], c["edges"], max_iterations=1)[5] in (binding.OK, binding.W_NOT_CONVERGED)


def test_descending_edge_list(ctx):
    g = pc.graph(9, [(i + 1, i) for i in range(8)] + [(8, 0), (5, 1)], 16)
    kw = dict(max_iterations=10)
    want = pm.optimize(g["poses"], g["edges"], **kw)
    rev = pm.optimize(g["poses"], g["edges"], reverse=True, **kw)
    s_graph = float(np.abs(want["poses"] - rev["poses"]).max())
    Pa, ra = ctx.pose_graph_optimize(g["poses"], g["edges"], **kw)[:2]
    Pd, rd, wd = ctx.pose_graph_optimize(g["poses"], g["edges"][::-1], **kw)[:3]
    print(f"descending edge list: ascending vs descending {np.abs(Pa - Pd).max():.3e}, bound {16 * s_graph:.3e}")
    assert np.abs(Pa - Pd).max() <= 16 * s_graph
    _compare("descending", Pd, rd, want, s_graph)


# ---- what the call leaves alone --------------------------------------------------------------------------------------
def _views(n_views=5, n_points=2000, seed=21):
    rng = np.random.default_rng(seed)
    world = rng.uniform(-1.0, 1.0, (3, n_points)) * np.array([[1.0], [0.7], [0.4]])
    truth, clouds = [], []
    for k in range(n_views):
        d = np.concatenate([np.radians(2.0) * k * np.array([0.3, 1.0, -0.5]), 0.02 * k * np.array([1.0, -0.5, 0.3])])
        P = pm.exp_pose(d)
        keep = rng.permutation(n_points)[:int(0.7 * n_points)]
        local = pm.inv_pose(P)[:3, :3] @ world[:, keep] + pm.inv_pose(P)[:3, 3:4]
        clouds.append((local + rng.normal(0.0, 0.001, local.shape)).astype(np.float32))
        truth.append(P)
    return np.array(truth), clouds


def test_the_context_is_left_alone(ctx):
    truth, clouds = _views(2)
    c = pc.case("A")

    def run(cx, optimise):
        cx.set_target(clouds[0])
        cx.set_source(clouds[1])
        T1 = cx.align(max_iterations=5, max_nn_dist=0.1)[0]
        if optimise:
            cx.pose_graph_optimize(c["poses"], c["edges"])
        src, (idx, dist) = cx.get_source(), cx.get_associations()
        T2 = cx.align(max_iterations=5, max_nn_dist=0.1)[0]
        return T1.tobytes(), src.tobytes(), idx.tobytes(), dist.tobytes(), T2.tobytes()

    with binding.Context(0) as plain:
        assert run(ctx, True) == run(plain, False)


def test_from_clouds(ctx):
    truth, clouds = _views()
    g = PoseGraph()
    g.add_node(truth[0])
    infos = []

    def align(s, t):
        ctx.set_target(clouds[t])
        ctx.set_source(clouds[s])
        T, st, rc = ctx.align(solve=binding.SOLVE_KABSCH, max_iterations=40, max_nn_dist=0.1)
        assert rc == binding.OK
        return np.asarray(T, np.float64).reshape(4, 4)

    def enter(s, t, T, uncertain):  # (the context still holds s as source and t as target)
        g.add_alignment(ctx, s, t, T, max_dist=0.05, uncertain=uncertain)
        sc = ctx.score_poses(T.astype(np.float32).reshape(1, 4, 4), max_dist=0.05)
        infos.append(binding.information_matrix(sc["sums"][0], sc["inliers"][0]))

    for k in range(1, 5):
        T = align(k, k - 1)
        g.add_node(g.poses()[k - 1] @ T)
        enter(k, k - 1, T, False)
    for s, t in ((4, 0), (3, 1)):
        enter(s, t, align(s, t), True)
    for e, (sums, inliers) in enumerate(g.scores):
        assert np.array_equal(g.edges[e][3], binding.information_matrix(sums, inliers))
        assert np.array_equal(g.edges[e][3], infos[e]) and inliers > 100
    start = g.poses()
    kw = dict(preference_loop_closure=2.0)
    want = pm.optimize(start, g.edges, **kw)
    rev = pm.optimize(start, g.edges, reverse=True, **kw)
    s_graph = float(np.abs(want["poses"] - rev["poses"]).max())
    res = g.optimize(ctx, **kw)
    print(f"from clouds: error against the truth {pc.pose_error(start, truth):.5f} -> {pc.pose_error(g.poses(), truth):.5f}; "
          f"cost {res.initial_cost:.6g} -> {res.final_cost:.6g}")
    assert res.final_cost <= res.initial_cost
    assert g.status == binding.OK and g.weights.shape == (6,) and not g.pruned.any()
    _compare("from clouds", g.poses(), res, want, s_graph)
