"""TEST INFRASTRUCTURE shared by the K16 tests (tests/test_fpfh_host.py, tests/test_gpu_fpfh.py, test_gpu_match.py,
test_gpu_global.py, test_gpu_fpfh_cpp.py): host normals for any cloud and the cluttered scene of the end-to-end case.
Normals always come from the host in these tests: the device estimate (K12) is not bit-equal to numpy, and the tests
are about K16."""
import numpy as np

from icp_slam_prototype_amd import synth


def host_normals(pts, radius, viewpoint=(0.0, 0.0, 0.0), min_neighbors=5):
    """(3, n) float32: the eigenvector of the smallest eigenvalue of the covariance of the neighbours within `radius`
    (the point included), turned towards `viewpoint`; (0, 0, 0) with fewer than min_neighbors or a non-finite point"""
    p = np.asarray(pts, np.float32).astype(np.float64).T
    n = len(p)
    out = np.zeros((n, 3))
    fin = np.isfinite(p).all(1)
    vp = np.asarray(viewpoint, np.float64)
    q = np.where(fin[:, None], p, 1e30)
    for a in range(0, n, 1024):
        d2 = ((q[a:a + 1024, None, :] - q[None, :, :]) ** 2).sum(-1)
        for r, i in enumerate(range(a, min(a + 1024, n))):
            if not fin[i]:
                continue
            nb = q[d2[r] <= radius * radius]
            if len(nb) < min_neighbors:
                continue
            w, v = np.linalg.eigh(np.cov(nb.T))
            e = v[:, 0]
            out[i] = -e if e @ (vp - p[i]) < 0 else e
    return np.ascontiguousarray(out.T.astype(np.float32))


def quarter_room():
    """about 3000 points: the quarter-resolution synthetic room (gicp_model.quarter_pair), both clouds with host normals"""
    import gicp_model as gm

    p = gm.quarter_pair()
    step = 4  # every fourth pixel of the 106 x 128 frame that is valid
    src = np.ascontiguousarray(p["source"][:, ::step])
    tgt = np.ascontiguousarray(p["target"][:, ::step])
    return dict(source=src, target=tgt, ns=host_normals(src, 0.25, (5, 5, 5)), nt=host_normals(tgt, 0.25, (5, 5, 5)))


def _box(rng, centre, size, n):
    """n points on the surface of an axis-aligned box"""
    c, s = np.asarray(centre, np.float64), np.asarray(size, np.float64)
    face = rng.integers(0, 6, n)
    u = rng.uniform(-0.5, 0.5, (n, 3)) * s
    ax, side = face // 2, (face % 2) - 0.5
    u[np.arange(n), ax] = side * s[ax]
    return c + u


def clutter_scene(seed=3, n_plane=500, n_clutter=1100):
    """A corner of a room (floor and two walls) with asymmetric clutter -- boxes and spheres of different sizes at
    irregular places -- as (n, 3) float64 world points.  The plain room of synth is three planes and a sphere: too
    planar for descriptors to tell places apart."""
    rng = np.random.default_rng(seed)
    parts = []
    for axis in range(3):  # the planes x = 0, y = 0, z = 0 over [0, 2]^2
        q = rng.uniform(0.0, 2.0, (n_plane, 3))
        q[:, axis] = 0.0
        parts.append(q)
    boxes = [((0.45, 0.35, 0.2), (0.5, 0.3, 0.4)), ((1.5, 0.5, 0.35), (0.3, 0.6, 0.7)), ((0.8, 1.5, 0.15), (0.9, 0.25, 0.3)),
             ((0.25, 1.2, 1.0), (0.5, 0.4, 0.2)), ((1.4, 0.15, 1.3), (0.45, 0.3, 0.35))]
    per = n_clutter // (len(boxes) + 2)
    for c, s in boxes:
        parts.append(_box(rng, c, s, per))
    for c, r in (((1.3, 1.3, 0.45), 0.3), ((0.5, 0.6, 0.75), 0.18)):
        v = rng.normal(0, 1, (per, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        v[:, 2] = np.abs(v[:, 2]) if c[2] < 0.5 else v[:, 2]
        parts.append(np.asarray(c) + r * v)
    return np.concatenate(parts)


def e2e_pair(seed=3, rot_deg=(25.0, -40.0, 60.0), shift=(0.4, -0.3, 0.25), keep=0.85, noise=0.0005, n_plane=500,
             n_clutter=1100, normal_radius=0.12):
    """The end-to-end pair: target and source are different random subsets of the cluttered scene with independent
    noise; the source is the scene moved by the INVERSE of the true pose, so that T_true (row-major 4 x 4 float64)
    moves source onto target.  Normals from the host, turned towards a viewpoint that moves with each cloud."""
    rng = np.random.default_rng(seed + 100)
    world = clutter_scene(seed, n_plane, n_clutter) + 5.0  # (the library's clouds live around (5, 5, 5))
    R = synth.rot_xyz_deg(*rot_deg)
    t = np.asarray(shift, np.float64) + 5.0 - R @ np.full(3, 5.0)  # a rotation about (5, 5, 5), then the shift
    tw = world[rng.random(len(world)) < keep]
    tw = tw + rng.normal(0, noise, tw.shape)
    sw = world[rng.random(len(world)) < keep]
    sw = sw + rng.normal(0, noise, sw.shape)
    sw = (sw - t) @ R  # R^T (p - t), row vectors
    vp_t = np.array([6.5, 6.5, 6.5])
    vp_s = R.T @ (vp_t - t)
    tgt = np.ascontiguousarray(tw.T.astype(np.float32))
    src = np.ascontiguousarray(sw.T.astype(np.float32))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return dict(source=src, target=tgt, ns=host_normals(src, normal_radius, vp_s), nt=host_normals(tgt, normal_radius, vp_t),
                T_true=T)
