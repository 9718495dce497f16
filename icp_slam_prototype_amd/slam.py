"""Closing loops (K30): the join between the fern keyframes that say "I have seen this before" (K27), the projective
alignment against a view built from one frame (K28), the pose graph with its line process (K18) and the TSDF volume,
which TsdfVolume.refuse can now correct without a reset.

    vol = TsdfVolume(ctx, ...)
    closer = LoopCloser(vol, frame_shape)
    for depth in frames:
        pose = tracker.track(depth)                 # any tracker; here one that fuses the frame itself
        closer.add(depth, pose, fused=True)
    r = closer.close()                              # optimise, re-fuse what moved, rewrite the keyframes' poses
    tracker.pose = r["pose"]

Frames live in host memory (depth, intensity, the pose they were fused at); no cap on their number is built."""
import numpy as np

from . import binding
from . import depth as depth_front
from .posegraph import PoseGraph


def correction_reach(old, new, z_max):
    """A bound on how far the correction old -> new moves a point of the frame's frustum: |dt| + 2 sin(dtheta / 2) z_max,
    with (dR, dt) = old^-1 new and z_max the frame's largest depth in metres."""
    E = np.linalg.inv(old) @ new
    c = np.clip((np.trace(E[:3, :3]) - 1) / 2, -1, 1)
    return float(np.linalg.norm(E[:3, 3]) + 2 * np.sqrt((1 - c) / 2) * z_max)  # (sin(t / 2) = sqrt((1 - cos t) / 2))


class LoopCloser:
    """A mapper on top of any tracker.  It owns the context's fern database, a PoseGraph and the record of every fused
    frame: depth, intensity, the pose it was fused at, its node and its pose relative to that node.

    pyramid: iteration counts per level, finest first, of the verification's coarse-to-fine projective loop.
    fern: FernParams fields (level default: the coarsest pyramid level).
    min_gap: a returned keyframe is a loop candidate when its node is at least this many nodes old ...
    max_diss: ... and its dissimilarity to the frame is at most this.
    min_overlap, max_mean_dist: K27's acceptance test on the verification's level 0: status OK, count >= min_overlap *
        (the frame's valid pixels), mean_dist <= max_mean_dist.
    projective: ProjectiveParams fields of the verification (max_dist, min_normal_cos, min_pairs).
    edge_level, edge_max_dist: an edge's information matrix is that of the two frames' clouds at this pyramid level
        (depth.backproject_level: the edge's s as the context's source, its t as the target) within edge_max_dist under
        T_st (PoseGraph.add_alignment: the convention the graph's other users have)."""

    def __init__(self, vol, shape, pyramid=(10, 5, 4), fern=None, min_gap=4, max_diss=None, min_overlap=0.3,
                 max_mean_dist=0.05, projective=None, edge_level=1, edge_max_dist=0.1, k=3):
        self.vol, self.ctx = vol, vol.ctx
        self.counts = tuple(int(n) for n in pyramid)
        self.pyramid_params = depth_front.pyramid_params(levels=len(self.counts))
        fern = dict(fern or {})
        fern.setdefault("level", len(self.counts) - 1)
        shapes = depth_front.pyramid_shapes(shape, len(self.counts))
        self.reloc = depth_front.Relocaliser(self.ctx, shapes[fern["level"]], **fern)
        self.min_gap = int(min_gap)
        self.max_diss = self.reloc.params.harvest_above if max_diss is None else int(max_diss)
        self.min_overlap, self.max_mean_dist = float(min_overlap), float(max_mean_dist)
        self.projective = dict(projective or {})
        self.projective.setdefault("max_dist", 0.5)
        self.edge_level, self.edge_max_dist, self.k = int(edge_level), float(edge_max_dist), int(k)
        self.graph = PoseGraph()
        self.frames = []         # dict(depth, intensity, pose, node, rel)
        self.node_frame = []     # node -> the frame that is the node
        self.keyframe_node = []  # fern keyframe -> node
        self.loop_edges = []     # indices into graph.edges of the accepted loop edges
        self.candidates = self.rejected = 0
        self.last_stats = None

    # -- the graph ------------------------------------------------------------------
    def _pyramid(self, frame):
        depth_front.build_pyramid(self.ctx, frame["depth"], self.pyramid_params)

    def _edge(self, s, t, T, uncertain):
        """the edge (s, t, T_st) between two nodes, its information from the two frames' clouds"""
        fx, cx = self.vol.fx, self.vol.cx
        self._pyramid(self.frames[self.node_frame[t]])
        depth_front.backproject_level(self.ctx, self.edge_level, which=1, fx=fx, cx=cx)
        self._pyramid(self.frames[self.node_frame[s]])
        depth_front.backproject_level(self.ctx, self.edge_level, which=0, fx=fx, cx=cx)
        return self.graph.add_alignment(self.ctx, s, t, T, max_dist=self.edge_max_dist, uncertain=uncertain)

    def _make_node(self, index):
        """frame `index` becomes a node (if it is none yet) with an odometry edge to the node before it, T from the
        given poses"""
        frame = self.frames[index]
        if frame["node"] is not None and self.node_frame[frame["node"]] == index:
            return frame["node"]
        node = self.graph.add_node(frame["pose"])
        self.node_frame.append(index)
        frame["node"], frame["rel"] = node, np.eye(4)
        if node > 0:
            prev = self.graph.poses()[node - 1]
            self._edge(node, node - 1, np.linalg.inv(prev) @ frame["pose"], uncertain=False)
        return node

    def _verify(self, frame, old_node, pose):
        """ProjectiveOdometry's alignment of `frame` against the view of the old keyframe at its current graph pose,
        from `pose`.  Returns (accepted, aligned pose)."""
        ctx, fx, cx = self.ctx, self.vol.fx, self.vol.cx
        self._pyramid(self.frames[self.node_frame[old_node]])
        valid_view, _ = binding.frame_view_build(ctx, self.graph.poses()[old_node], fx=fx, cx=cx)
        self._pyramid(frame)
        estimate, st = np.array(pose, np.float64), None
        try:
            for l in range(len(self.counts) - 1, -1, -1):
                p = binding.default_projective_params(**dict(self.projective, level=l, fx=fx, cx=cx, max_iterations=self.counts[l]))
                if valid_view[l] < p.min_pairs:
                    if l == 0:
                        return False, estimate
                    continue
                binding.projective_set_view(ctx, binding.VIEW_FRAME, l)
                estimate, st = binding.align_projective(ctx, estimate, p)
        finally:
            binding.projective_set_view(ctx, binding.VIEW_RAYCAST)
        self.last_stats = st
        valid = int(np.count_nonzero(frame["depth"]))
        ok = st is not None and st.status == binding.OK and st.count >= self.min_overlap * valid and \
            st.mean_dist <= self.max_mean_dist
        return bool(ok), estimate

    # -- the two calls --------------------------------------------------------------
    def add(self, depth, pose, intensity=None, fused=False):
        """One frame at the tracker's camera-to-world pose.  fused: the tracker has fused it already.  Returns
        dict(node (or None), keyframe (or -1), loops: the nodes an accepted loop edge now joins the frame's node to)."""
        depth = np.ascontiguousarray(depth, np.uint16)
        pose = np.array(pose, np.float64).reshape(4, 4)
        frame = dict(depth=depth, intensity=None if intensity is None else np.ascontiguousarray(intensity, np.float32),
                     pose=pose, node=None, rel=None)
        self._pyramid(frame)
        if not fused:
            self.vol.integrate(depth, pose, frame["intensity"])
        r = binding.fern_process(self.ctx, pose, self.k)
        index = len(self.frames)
        self.frames.append(frame)
        harvested = r["added"] >= 0
        if harvested or not self.node_frame:  # (the first frame is a node whatever the ferns say: node 0 is the anchor)
            node = self._make_node(index)
            if harvested:
                self.keyframe_node.append(node)
        else:
            last = self.graph.n_nodes - 1
            frame["node"], frame["rel"] = last, np.linalg.inv(self.graph.poses()[last]) @ pose
        loops = []
        for kf, diss in zip(r["index"], r["diss"]):
            old = self.keyframe_node[int(kf)]
            if self.graph.n_nodes - 1 - old < self.min_gap or diss > self.max_diss or old in loops:
                continue
            self.candidates += 1
            ok, aligned = self._verify(frame, old, pose)
            if not ok:
                self.rejected += 1
                continue
            node = self._make_node(index)
            T = np.linalg.inv(self.graph.poses()[old]) @ aligned
            self.loop_edges.append(self._edge(node, old, T, uncertain=True))
            loops.append(old)
        return dict(node=frame["node"] if self.node_frame[frame["node"]] == index else None, keyframe=int(r["added"]),
                    loops=loops)

    def close(self, **pg_kw):
        """Optimises the graph (PG_PRUNE on, node 0 fixed), gives every frame the pose P_node . rel, re-fuses exactly the
        frames whose correction can move a point of their frustum by more than half a voxel, and rewrites the fern
        database's poses.  Returns dict(pose: the corrected latest pose, edges_accepted, edges_pruned, frames_refused,
        refused: their indices)."""
        if not self.frames:
            raise ValueError("no frame has been added")
        pg_kw.setdefault("reference_node", 0)
        # (0, the library's default, leaves the line process off.  A loop edge's chi2 at the odometry-only state is the
        # drift squared in units of the edge's information: 200 .. 470 on the room loop at 6 deg / 83 mm, where 2 prunes
        # the true closures with the false ones and 100 keeps them -- DESIGN.md K30 has the table)
        pg_kw.setdefault("preference_loop_closure", 100.0)
        pg_kw["flags"] = int(pg_kw.get("flags", 0)) | binding.PG_PRUNE
        self.graph.optimize(self.ctx, **pg_kw)
        nodes = self.graph.poses()
        p = self.vol.params
        moved, old, new = [], [], []
        for k, f in enumerate(self.frames):
            corrected = nodes[f["node"]] @ f["rel"]
            z_max = float(f["depth"].max()) / p.depth_scale
            if correction_reach(f["pose"], corrected, z_max) > 0.5 * p.voxel:
                moved.append(k), old.append(f["pose"]), new.append(corrected)
        if moved:
            color = self.frames[moved[0]]["intensity"] is not None
            self.vol.refuse([self.frames[k]["depth"] for k in moved], old, new,
                            [self.frames[k]["intensity"] for k in moved] if color else None)
            for k, P in zip(moved, new):
                self.frames[k]["pose"] = P
        codes = [binding.fern_keyframe(self.ctx, i)[0] for i in range(len(self.keyframe_node))]
        binding.fern_reset(self.ctx)
        for code, node in zip(codes, self.keyframe_node):
            binding.fern_add_code(self.ctx, code, nodes[node])
        pruned = int(sum(bool(self.graph.pruned[e]) for e in self.loop_edges))
        last = self.frames[-1]
        return dict(pose=nodes[last["node"]] @ last["rel"], edges_accepted=len(self.loop_edges), edges_pruned=pruned,
                    frames_refused=len(moved), refused=moved)
