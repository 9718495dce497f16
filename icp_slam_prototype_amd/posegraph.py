"""Multiway registration (K18): a pose graph of pairwise alignments, each weighted by its information matrix, optimised
on the device by Context.pose_graph_optimize (Levenberg-Marquardt, with a line process that switches wrong loop
closures off).

    g = PoseGraph()
    g.add_node(np.eye(4))
    for k in range(1, n):                      # odometry: frame k aligned onto frame k - 1
        ctx.set_target(cloud[k - 1]); ctx.set_source(cloud[k])
        T, st, rc = ctx.align()
        g.add_node(g.poses()[k - 1] @ T)       # the chained pose: P_k = P_{k-1} T_{k, k-1}
        g.add_alignment(ctx, k, k - 1, T, max_dist=0.05)
    ...                                        # a loop closure found by ctx.register_global + ctx.align:
    g.add_alignment(ctx, s, t, T_st, max_dist=0.05, uncertain=True)
    result = g.optimize(ctx, preference_loop_closure=2.0, flags=binding.PG_PRUNE)
"""
import numpy as np

from . import binding


class PoseGraph:
    """Nodes P_i (4 x 4, node i's cloud into the world) and edges (s, t, T_st, info, uncertain): T_st moves cloud s onto
    cloud t -- what Context.align returns with s as source and t as target -- and is satisfied when P_s = P_t T_st."""

    def __init__(self):
        self._poses = []
        self.edges = []
        self.scores = []     # per add_alignment call: the (sums, inliers) its information matrix was made of
        self.weights = None  # per edge, after optimize: the line process's l ...
        self.chi2 = None     # ... the edge's chi2 ...
        self.pruned = None   # ... and whether PG_PRUNE dropped it
        self.status = None   # OK or W_NOT_CONVERGED

    @property
    def n_nodes(self):
        return len(self._poses)

    @property
    def n_edges(self):
        return len(self.edges)

    def add_node(self, P):
        P = np.array(P, np.float64)
        if P.shape != (4, 4):
            raise ValueError("a pose is a 4 x 4 matrix")
        self._poses.append(P)
        return len(self._poses) - 1

    def add_edge(self, s, t, T, info, uncertain=False):
        T, info = np.array(T, np.float64), np.array(info, np.float64)
        if T.shape != (4, 4) or info.shape != (6, 6):
            raise ValueError("an edge needs a 4 x 4 transform and a 6 x 6 information matrix")
        if not (0 <= s < self.n_nodes and 0 <= t < self.n_nodes) or s == t:
            raise ValueError("an edge joins two different nodes of the graph")
        self.edges.append((int(s), int(t), T, info, bool(uncertain)))
        return len(self.edges) - 1

    def add_alignment(self, ctx, s, t, T, max_dist, uncertain=False):
        """The edge of an alignment the context has just made: it holds cloud s as its source and cloud t as its target.
        The information matrix is that of the pairs within max_dist under T (Context.score_poses +
        binding.information_matrix)."""
        sc = ctx.score_poses(np.asarray(T, np.float32).reshape(1, 4, 4), max_dist=max_dist)
        info = binding.information_matrix(sc["sums"][0], sc["inliers"][0])
        self.scores.append((sc["sums"][0].copy(), int(sc["inliers"][0])))
        return self.add_edge(s, t, T, info, uncertain)

    def poses(self):
        return np.array(self._poses, np.float64).reshape(-1, 4, 4)

    def optimize(self, ctx, params=None, **kw):
        """Context.pose_graph_optimize over the graph; the poses are replaced by the optimised ones.  Returns the
        PgResult and keeps weights, chi2, pruned and status."""
        P, res, self.weights, self.chi2, self.pruned, self.status = ctx.pose_graph_optimize(self.poses(), self.edges,
                                                                                            params, **kw)
        self._poses = [P[i].copy() for i in range(P.shape[0])]
        return res
