"""Pose-graph optimisation (K18) on the CPU: the model of tests/posegraph_model.py against central differences and
against scipy.optimize.least_squares, the rule's series against libm, the graphs' sensitivity to summation order, the
pruning that would cut a node off, and the host-side refusals of the C ABI (icpk_pose_graph_check: the argument checks
both device calls start with, which need no device)."""
import ctypes as C
import math

import numpy as np
import pytest

import posegraph_cases as pc
import posegraph_model as pm
from icp_slam_prototype_amd import binding, build


@pytest.fixture(scope="module")
def lib():
    build.build()
    return binding.load()


# ---- Jacobians -------------------------------------------------------------------------------------------------------
def _random_pose(rng, max_angle):
    w = rng.normal(size=3)
    w *= rng.uniform(0.0, max_angle) / np.linalg.norm(w)
    P = np.eye(4)
    P[:3, :3] = pm.rot_exp(w)
    P[:3, 3] = rng.uniform(-3.0, 3.0, 3)
    return P


def _numeric_jacobians(Ps, Pt, T, h):
    Js, Jt = np.zeros((6, 6)), np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        Js[:, k] = (pm.residual(pm.exp_pose(d) @ Ps, Pt, T)[0] - pm.residual(pm.exp_pose(-d) @ Ps, Pt, T)[0]) / (2 * h)
        Jt[:, k] = (pm.residual(Ps, pm.exp_pose(d) @ Pt, T)[0] - pm.residual(Ps, pm.exp_pose(-d) @ Pt, T)[0]) / (2 * h)
    return Js, Jt


# Central differences with h = 1e-6: the truncation error is h^2 / 6 times a third derivative of order |t_B| <= 10, so
# 2e-11; the rounding error is eps |r| / h with |r| <= 10: 2e-9.  The bound is 1e-7 (fifty times the larger), far below
# the 0.1 .. 0.5 by which J with Jl^-1 taken as I would be off at these rotations.
JAC_TOL = 1e-7


def test_model_jacobians_equal_central_differences():
    rng = np.random.default_rng(5)
    worst = 0.0
    for k in range(50):
        Ps, Pt = _random_pose(rng, 3.0), _random_pose(rng, 3.0)
        # the edge's error E has a rotation of up to 2 rad: T = E^-1-ish of a drawn error
        E = _random_pose(rng, 2.0)
        T = pm.inv_pose(E) @ pm.inv_pose(Pt) @ Ps
        r, tB = pm.residual(Ps, Pt, T)
        assert np.linalg.norm(r[:3]) <= 2.0 + 1e-9
        J = pm.jacobian_source(Pt, r, tB)
        Js, Jt = _numeric_jacobians(Ps, Pt, T, 1e-6)
        worst = max(worst, float(np.abs(J - Js).max()), float(np.abs(-J - Jt).max()))
    print(f"jacobians, 50 random edges: worst |analytic - numeric| = {worst:.3e}")
    assert worst < JAC_TOL
    # an approximation would show: Jl^-1 = I is off by about |theta| / 2
    assert np.abs(np.eye(3) - pm.jl_inv(np.array([0.3, -0.2, 0.5]))).max() > 0.1


def test_model_jacobians_at_zero_error():
    rng = np.random.default_rng(6)
    worst = 0.0
    for k in range(10):
        Ps, Pt = _random_pose(rng, 3.0), _random_pose(rng, 3.0)
        T = pm.inv_pose(Pt) @ Ps  # E = I up to rounding
        r, tB = pm.residual(Ps, Pt, T)
        assert np.abs(r).max() < 1e-14
        J = pm.jacobian_source(Pt, r, tB)
        Js, Jt = _numeric_jacobians(Ps, Pt, T, 1e-6)
        worst = max(worst, float(np.abs(J - Js).max()), float(np.abs(-J - Jt).max()))
    print(f"jacobians, E = I: worst |analytic - numeric| = {worst:.3e}")
    assert worst < JAC_TOL


# ---- the rule's series against libm ----------------------------------------------------------------------------------
# The device and the model share rod_coeffs, atan_pos and angle_pos operation for operation, so no device-against-model
# test can see an inaccuracy in them: libm is the independent reference here.  Bounds, from the roundings counted:
#   a = sin(th) / th, b = (1 - cos th) / th^2 (both <= 1): a Horner step is a division, a product and a subtraction (3
#   roundings of numbers <= 1: 1.5 eps) and the error of the steps inside it is scaled by th^2 / ((2k)(2k + 1)) <=
#   pi^2 / 6, pi^2 / 20, ...: 1.5 eps (1 + 1.65 (1 + 0.5 (1 + ...))) < 6 eps absolute for a, less for b.  Asserted: 8 eps
#   absolute (near th = pi, where a -> 0, no relative bound holds; Rodrigues uses a and b beside 1, so absolute counts).
#   atan: each of the three halvings is x * x, 1 +, sqrt, 1 +, / (<= 2.5 ulps of relative error in x, which atan passes
#   on at most as it is), the reciprocal above 1 half an ulp, the Horner sum about 2, the two closing products 1 and the
#   subtraction from pi/2 one more: < 13 ulps.  Asserted: 16 ulps of the result, for atan and for the angle of (c, s).
SERIES_ABS_TOL = 8 * np.finfo(np.float64).eps
ATAN_ULPS = 16


def test_series_of_the_rule_equal_libm():
    rng = np.random.default_rng(9)
    ths = np.concatenate([np.linspace(0.0, math.pi, 4001), rng.uniform(0.0, math.pi, 4000), 10.0 ** rng.uniform(-12, 0, 1000)])
    wa = wb = wang = wat = 0.0
    for th in ths:
        th = float(th)
        a, b = pm.rod_coeffs(th * th)
        ra = math.sin(th) / th if th > 0.0 else 1.0
        rb = 2.0 * math.sin(th / 2.0) ** 2 / (th * th) if th > 0.0 else 0.5  # (1 - cos th without its cancellation)
        wa, wb = max(wa, abs(a - ra)), max(wb, abs(b - rb))
        s, c = math.sin(th), math.cos(th)
        if s > 0.0 or c > 0.0:  # (what rot_log asks of angle_pos)
            ref = math.atan2(s, c)
            if ref > 0.0:
                wang = max(wang, abs(pm.angle_pos(s, c) - ref) / np.spacing(ref))
    for x in np.concatenate([10.0 ** rng.uniform(-10, 10, 8000), [1.0, 0.5, 2.0]]):
        ref = math.atan(float(x))
        wat = max(wat, abs(pm.atan_pos(float(x)) - ref) / np.spacing(ref))
    eps = np.finfo(np.float64).eps
    print(f"series vs libm on [0, pi]: sin(th)/th {wa / eps:.2f} eps, (1 - cos th)/th^2 {wb / eps:.2f} eps, "
          f"angle {wang:.1f} ulps, atan {wat:.1f} ulps")
    assert pm.atan_pos(0.0) == 0.0 and pm.rod_coeffs(0.0) == (1.0, 0.5)
    assert wa <= SERIES_ABS_TOL and wb <= SERIES_ABS_TOL
    assert wang <= ATAN_ULPS and wat <= ATAN_ULPS
    # Rodrigues of the series is a rotation up to 2 pi (the header: "usable to 2 pi")
    for th in (1e-9, 0.5, math.pi, 6.0, 2.0 * math.pi):
        R = pm.rot_exp(th * np.array([0.6, -0.48, 0.64]))
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12


# ---- the optimum against scipy ---------------------------------------------------------------------------------------
def _plain_residual(Ps, Pt, T):
    """the residual of the rule written the ordinary way (numpy products, libm's atan2): scipy's reference does not share
    the model's fixed-order arithmetic"""
    E = np.linalg.inv(Pt) @ Ps @ np.linalg.inv(T)
    R = E[:3, :3]
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = np.linalg.norm(v), 0.5 * (np.trace(R) - 1.0)
    w = v * (np.arctan2(s, c) / s) if s > 1e-12 else v
    return np.concatenate([w, E[:3, 3]])


def _scipy_optimum(poses, edges, mu, ref=0):
    from scipy.optimize import least_squares

    n = len(poses)
    free = [i for i in range(n) if i != ref]
    chol = [np.linalg.cholesky(ed[3]) for ed in edges]  # info = C C^T: chi2 = |C^T r|^2

    def unpack(x):
        P = np.array(poses)
        for k, i in enumerate(free):
            P[i] = pm.exp_pose(x[6 * k:6 * k + 6]) @ poses[i]
        return P

    def fun(x):
        P = unpack(x)
        out = []
        for (s, t, T, info, unc), Cc in zip(edges, chol):
            w = Cc.T @ _plain_residual(P[s], P[t], T)
            if unc and mu > 0.0:
                sl = mu / (mu + float(w @ w))  # sqrt(l)
                out.append(sl * w)
                out.append([np.sqrt(mu) * (sl - 1.0)])
            else:
                out.append(w)
        return np.concatenate(out)

    res = least_squares(fun, np.zeros(6 * len(free)), method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
    return unpack(res.x), 2.0 * res.cost


def _scipy_case(name):
    c = pc.case(name)
    mu = c["params"].get("preference_loop_closure", 0.0)
    P, cost = _scipy_optimum(c["poses"], c["edges"], mu)
    if c["params"].get("prune"):
        l = pm.edge_pass(P, c["edges"], mu, blocks=False)[1]
        kept = [ed for e, ed in enumerate(c["edges"]) if not (ed[4] and l[e] < 0.25)]
        P, cost = _scipy_optimum(P, kept, mu)
    return P, cost


# Measured here (model against scipy 1.15, trf, tolerances 1e-15): largest pose difference and relative cost difference
#   case A  2.9e-09 / 7.9e-15    case B  1.3e-09 / 5.2e-15    case C  1.6e-08 / 6.4e-14
# The model stops on a relative cost decrease of 1e-9 and scipy on its own criteria, so the two optima differ by what
# the last model step would still have moved.  The test asserts 8 x the largest measured figure of each kind.
SCIPY_POSE_TOL = 8 * 1.6e-08
SCIPY_COST_TOL = 8 * 6.4e-14


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_model_optimum_equals_scipy(name):
    r = pc.model_result(name)
    P, cost = _scipy_case(name)
    dp = float(np.abs(r["poses"] - P).max())
    dc = abs(r["final_cost"] - cost) / cost
    print(f"case {name}: model vs scipy: pose {dp:.3e}, relative cost {dc:.3e}; model cost {r['final_cost']:.12g}")
    assert r["converged"]
    assert dp < SCIPY_POSE_TOL and dc < SCIPY_COST_TOL
    if name == "C":
        e = [k for k, ed in enumerate(pc.case("C")["edges"]) if (ed[0], ed[1]) == pc.FALSE_CLOSURE]
        assert list(np.nonzero(r["pruned"])[0]) == e and r["n_pruned"] == 1


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_rounding_sensitivity_is_what_the_cases_record(name):
    """s_graph: the model with every node's gather order reversed.  A node with two incident edges sums two terms, which
    does not depend on their order, so only the nodes with three can differ at all: the ends of the closures (8 in
    cases B and C, 3 and 11 as well in C; node 0 has three too, but it is the reference node and its sums go unused)."""
    s = pc.s_graph(name)
    print(f"case {name}: s_graph = {s:.3e}")
    assert s <= pc.S_GRAPH[name]


def test_model_prunes_nothing_when_that_would_cut_a_node_off():
    """The rule (include/icpk.h, "pruning"): edges whose loss would leave a node without a way to the reference node are
    not dropped.  With a threshold above 1 every uncertain edge qualifies (l <= 1); in the first graph the uncertain edge
    is a bridge, in the second a closure."""
    g, kw = pc.prune_bridge_graph()
    r = pm.optimize(g["poses"], g["edges"], **kw)
    plain = pm.optimize(g["poses"], g["edges"], **dict(kw, prune=False))
    assert not r["pruned"].any() and r["n_pruned"] == 0
    assert r["iterations"] == plain["iterations"] and r["poses"].tobytes() == plain["poses"].tobytes()
    assert not pm.connected(5, [ed for ed in g["edges"] if not ed[4]], 0)
    # the same threshold where the uncertain edge is a closure: it goes, and a second run follows
    c = pc.graph(5, [(1, 0), (2, 1), (3, 2), (4, 3), (4, 0)], 31, uncertain=(4,))
    r = pm.optimize(c["poses"], c["edges"], **kw)
    assert list(r["pruned"]) == [False] * 4 + [True] and r["n_pruned"] == 1


# ---- host-side refusals ----------------------------------------------------------------------------------------------
def test_every_refusal_of_the_rule_is_made_on_the_host(lib):
    c = pc.case("A")
    P, E = c["poses"], c["edges"]
    ok = binding.OK
    assert binding.pose_graph_check(P, E) == ok
    bad = binding.E_ARG
    # null pointers
    assert binding.pose_graph_check(None, E, n_nodes=8) == bad
    assert binding.pose_graph_check(P, None, n_edges=8) == bad
    # sizes
    assert binding.pose_graph_check(P[:1], E[:1]) == bad
    assert binding.pose_graph_check(P, E, n_edges=0) == bad
    assert binding.pose_graph_check(P, E, n_nodes=binding.PG_MAX_NODES + 1) == bad
    assert binding.pose_graph_check(P, E, n_edges=binding.PG_MAX_EDGES + 1) == bad

    def with_edge(k, **kw):
        s, t, T, info, u = E[k]
        d = dict(s=s, t=t, T=T, info=info)
        d.update(kw)
        return E[:k] + [(d["s"], d["t"], d["T"], d["info"], u)] + E[k + 1:]

    assert binding.pose_graph_check(P, with_edge(2, s=E[2][1])) == bad  # s == t
    assert binding.pose_graph_check(P, with_edge(2, s=8)) == bad
    assert binding.pose_graph_check(P, with_edge(2, t=-1)) == bad
    for v in (np.nan, np.inf):
        T = E[3][2].copy()
        T[1, 3] = v
        assert binding.pose_graph_check(P, with_edge(3, T=T)) == bad
        info = E[3][3].copy()
        info[5, 0] = v
        assert binding.pose_graph_check(P, with_edge(3, info=info)) == bad
        Q = P.copy()
        Q[7, 0, 0] = v
        assert binding.pose_graph_check(Q, E) == bad
    # a node the reference node cannot reach: without the odometry edge 4 -> 3 the closure 7 -> 0 still joins the two
    # halves; without both, nodes 4 .. 7 hang free
    assert binding.pose_graph_check(P, E[:3] + E[4:]) == ok
    assert binding.pose_graph_check(P, E[:3] + E[4:7]) == bad
    # parameters
    assert binding.pose_graph_check(P, E, binding.default_pg_params(reference_node=7)) == ok
    assert binding.pose_graph_check(P, E, binding.default_pg_params(reference_node=8)) == bad
    assert binding.pose_graph_check(P, E, binding.default_pg_params(flags=2)) == bad
    assert binding.pose_graph_check(P, E, binding.default_pg_params(tau=0.0)) == bad
    assert binding.pose_graph_check(P, E, binding.default_pg_params(pcg_tolerance=np.nan)) == bad
    # the device calls make the same checks, after the null context
    dp = C.POINTER(C.c_double)
    Pc = np.ascontiguousarray(P)
    assert lib.icpk_pose_graph_optimize(None, 8, Pc.ctypes.data_as(dp), len(E), binding.pg_edges(E), None, None, None,
                                        None, None) == bad
    assert lib.icpk_pose_graph_evaluate(None, 8, Pc.ctypes.data_as(dp), len(E), binding.pg_edges(E), 0.0, None, None, None,
                                        None) == bad
    n = C.c_int32(0)
    assert lib.icpk_get_pose_graph_trace(None, C.byref(n), None, None, None, None) == bad


def test_structures_and_defaults_match_the_header(lib):
    assert C.sizeof(binding.PgEdge) == 16 + 16 * 8 + 36 * 8
    assert C.sizeof(binding.PgParams) == 8 + 7 * 8 + 8
    assert C.sizeof(binding.PgResult) == 16 + 3 * 8
    p = binding.default_pg_params()
    assert (p.max_iterations, p.max_pcg_iterations, p.reference_node, p.flags) == (100, 200, 0, 0)
    assert (p.pcg_tolerance, p.tau, p.cost_tolerance, p.step_tolerance, p.gradient_tolerance) == (1e-8, 1e-3, 1e-9, 1e-10, 1e-10)
    assert (p.preference_loop_closure, p.edge_prune_threshold) == (0.0, 0.25)
    assert binding.W_NOT_CONVERGED == 4 and binding.PG_PRUNE == 1
    assert {k: v for k, v in pm.DEFAULTS.items() if k != "prune"} == \
        {k: getattr(p, k) for k in pm.DEFAULTS if k != "prune"}


def test_pose_graph_collects_nodes_and_edges():
    from icp_slam_prototype_amd.posegraph import PoseGraph

    c = pc.case("A")
    g = PoseGraph()
    for P in c["poses"]:
        g.add_node(P)
    for s, t, T, info, u in c["edges"]:
        g.add_edge(s, t, T, info, uncertain=u)
    assert g.n_nodes == 8 and g.n_edges == 8 and np.array_equal(g.poses(), c["poses"])
    assert binding.pose_graph_check(g.poses(), g.edges) == binding.OK
    with pytest.raises(ValueError):
        g.add_edge(0, 8, np.eye(4), np.eye(6))
    with pytest.raises(ValueError):
        g.add_node(np.eye(3))
