"""The pose graphs the K18 tests share (tests/test_posegraph_host.py, tests/test_gpu_posegraph*.py).

Poses lie on a ring of radius 2 m; node i looks along the tangent and has a small vertical wobble.  An edge's
measurement is the true relative pose perturbed on the left by N(0, 0.01 rad), N(0, 0.02 m) from a seeded generator;
its information matrix is sum G^T G, G = [-[q]x | I], over 40 seeded points of spread 1.5 m.  Odometry edge i joins
source i + 1 to target i; the initial poses are the chained odometry from the true pose of node 0.

  case A   8 nodes, 7 odometry edges and the closure 7 -> 0
  case B   16 nodes and the closures 15 -> 0 and 8 -> 0
  case C   B plus a false closure 11 -> 3 (the true relative pose displaced by (0.5, 0.3, -0.4) rad and
           (0.5, -0.3, 0.2) m); it runs with mu = 25 and pruning.  The closures are the uncertain edges.

Sensitivity to summation order (s_graph: the largest pose difference between the model's run and its run with every
node's gather order reversed), measured by tests/test_posegraph_host.py, which prints it.  A node with two incident
edges sums two terms, which does not depend on their order; only a free node with three or more can differ at all.
Those are the closures' ends: node 8 in cases B and C, nodes 3 and 11 as well in C (node 0 has three too, but it is the
reference node and its sums go unused).  Case A has none.
  case A   0
  case B   4.44e-16 (2 eps)
  case C   4.44e-16 (2 eps)
"""
import functools

import numpy as np

import posegraph_model as pm

# the figures of the docstring; the host test asserts that a fresh measurement is not above them
S_GRAPH = {"A": 0.0, "B": 2 * np.finfo(np.float64).eps, "C": 2 * np.finfo(np.float64).eps}
FALSE_CLOSURE = (11, 3)


def ring_poses(n):
    P = np.zeros((n, 4, 4))
    for i in range(n):
        a = 2.0 * np.pi * i / n
        yaw = a + np.pi / 2.0
        P[i] = np.eye(4)
        P[i, :3, :3] = [[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]]
        P[i, :3, 3] = [2.0 * np.cos(a), 2.0 * np.sin(a), 0.05 * np.sin(3.0 * a)]
    return P


def information(rng, points=40, spread=1.5):
    q = rng.normal(0.0, spread, (points, 3))
    info = np.zeros((6, 6))
    for p in q:
        G = np.hstack([-pm.skew(p), np.eye(3)])
        info += G.T @ G
    return info


def measured(rng, truth, s, t, offset=None):
    """T_st: P_t^-1 P_s, displaced by `offset` (6,) on the left if given, then by the noise on the left"""
    T = pm.inv_pose(truth[t]) @ truth[s]
    if offset is not None:
        T = pm.exp_pose(np.asarray(offset, np.float64)) @ T
    noise = np.concatenate([rng.normal(0.0, 0.01, 3), rng.normal(0.0, 0.02, 3)])
    return pm.exp_pose(noise) @ T


def chain(truth, edges):
    """the chained odometry: P_0 true, P_{i+1} = P_i T_{i+1, i}"""
    P = np.zeros_like(truth)
    P[0] = truth[0]
    for i in range(len(truth) - 1):
        s, t, T = edges[i][:3]
        assert (s, t) == (i + 1, i)
        P[i + 1] = P[i] @ T
    return P


def make_case(n, closures, seed, false_closure=None):
    rng = np.random.default_rng(seed)
    truth = ring_poses(n)
    edges = [(i + 1, i, measured(rng, truth, i + 1, i), information(rng), False) for i in range(n - 1)]
    for s, t in closures:
        edges.append((s, t, measured(rng, truth, s, t), information(rng), True))
    if false_closure is not None:
        s, t = false_closure
        edges.append((s, t, measured(rng, truth, s, t, offset=(0.5, 0.3, -0.4, 0.5, -0.3, 0.2)), information(rng), True))
    return dict(truth=truth, poses=chain(truth, edges), edges=edges)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(truth, poses, edges, params): params are the model's keywords (the binding's differ only in `prune`)"""
    if name == "A":
        c = make_case(8, [(7, 0)], seed=101)
        c["params"] = {}
    elif name == "B":
        c = make_case(16, [(15, 0), (8, 0)], seed=202)
        c["params"] = {}
    elif name == "C":
        c = make_case(16, [(15, 0), (8, 0)], seed=202, false_closure=FALSE_CLOSURE)
        c["params"] = dict(preference_loop_closure=25.0, prune=True)
    else:
        raise KeyError(name)
    return c


@functools.lru_cache(maxsize=None)
def model_result(name, reverse=False):
    """the model's optimum of a case, computed once and shared (treat it as read-only)"""
    c = case(name)
    return pm.optimize(c["poses"], c["edges"], reverse=reverse, **c["params"])


def s_graph(name):
    """a case's sensitivity to summation order, measured afresh from the two shared model runs"""
    return float(np.max(np.abs(model_result(name)["poses"] - model_result(name, True)["poses"])))


def binding_params(params):
    """the model's keywords as Context.pose_graph_optimize takes them"""
    from icp_slam_prototype_amd import binding

    kw = dict(params)
    if kw.pop("prune", False):
        kw["flags"] = binding.PG_PRUNE
    return kw


def pose_error(P, truth):
    """largest entry of P_i - truth_i over all nodes"""
    return float(np.max(np.abs(np.asarray(P) - truth)))


def graph(n, pairs, seed, uncertain=(), start_noise=(0.02, 0.04)):
    """a graph over the ring's poses with an edge per (s, t) of `pairs`; the initial poses are the true ones displaced on
    the left by N(0, start_noise) (rad, m) -- node 0 too"""
    rng = np.random.default_rng(seed)
    truth = ring_poses(n)
    edges = [(s, t, measured(rng, truth, s, t), information(rng), k in uncertain) for k, (s, t) in enumerate(pairs)]
    poses = np.array([pm.exp_pose(np.concatenate([rng.normal(0.0, start_noise[0], 3), rng.normal(0.0, start_noise[1], 3)]))
                      @ truth[i] for i in range(n)])
    return dict(truth=truth, poses=poses, edges=edges)


def prune_bridge_graph():
    """(graph, model keywords): a chain of 5 whose link 3 -> 2 is the one uncertain edge, with a prune threshold above 1,
    so that the line process offers the bridge for pruning (l <= 1 < threshold) and dropping it would cut 3 and 4 off"""
    g = graph(5, [(1, 0), (2, 1), (3, 2), (4, 3)], 30, uncertain=(2,))
    return g, dict(preference_loop_closure=25.0, edge_prune_threshold=2.0, prune=True)
