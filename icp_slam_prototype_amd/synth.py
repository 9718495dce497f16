"""Synthetic workloads for the BASELINE.json configs.

Pure numpy; used by bench.py and tests/.  No dataset ships with the reference
(CoRBS/TUM sequences are not fetchable), so every workload is generated:
depth images are ray-cast from a small analytic room and back-projected with
the reference's own formula (pointcloud.cpp:37-39, including its use of CX/FX
for the y axis) WITHOUT the rand()%40 subsample (pointcloud.cpp:28; the library's seeded stand-in is icpk_set_subsample).
"""
import numpy as np

# pointcloud.hpp:7-10
FX = np.float32(468.60)
FY = np.float32(468.61)
CX = np.float32(318.27)
CY = np.float32(243.99)
# SLAM.cpp:25-35,135 (Kinect v2 depth intrinsics)
K2_FX = np.float32(363.58)
K2_CX = np.float32(250.32)

CAMERA_START = np.float32(5.0)  # icp.cpp:53 cameraPosition = (5,5,5)


def rot_xyz_deg(x, y, z):
    """float64 restatement of the sign convention of icp.cpp:640-653 (Rx*Ry*Rz)."""
    ax, ay, az = np.deg2rad([x, y, z])
    rx = np.array([[1, 0, 0], [0, np.cos(ax), np.sin(ax)], [0, -np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, -np.sin(ay)], [0, 1, 0], [np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), np.sin(az), 0], [-np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return rx @ ry @ rz


def backproject(depth, keep=None, fx=FX, cx=CX):
    """numpy restatement of pointcloud.cpp:19-58 (float32 arithmetic, row-major
    order of the non-zero pixels).  Returns (3, N) float32 SoA."""
    depth = np.asarray(depth, np.uint16)
    m = depth != 0
    if keep is not None:
        m &= np.asarray(keep, bool)
    r, c = np.nonzero(m)  # row-major order
    d = depth[r, c].astype(np.float32)
    pz = d / np.float32(5000.0)
    px = (c.astype(np.float32) - np.float32(cx)) * pz / np.float32(fx)
    py = (r.astype(np.float32) - np.float32(cx)) * pz / np.float32(fx)
    return np.stack([px, py, pz]).astype(np.float32)


def render_room_depth(rows, cols, R_wc, c_w, fx=FX, cx=CX, noise_sigma=0.0, rng=None):
    """Ray-cast a room (floor, back wall, left wall, one sphere) from a camera
    with world-from-camera rotation R_wc and centre c_w.  Ray directions use the
    same pinhole the reference back-projects with, so back-projection of the
    result reproduces the hit points.  Returns uint16 depth = metres * 5000."""
    v, u = np.mgrid[0:rows, 0:cols].astype(np.float64)
    d_cam = np.stack([(u - float(cx)) / float(fx), (v - float(cx)) / float(fx), np.ones_like(u)], -1)
    w = d_cam @ np.asarray(R_wc, np.float64).T
    o = np.asarray(c_w, np.float64)
    t_best = np.full((rows, cols), np.inf)

    def plane(n, h):
        n = np.asarray(n, np.float64)
        den = w @ n
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (h - o @ n) / den
        t[~(t > 1e-6)] = np.inf
        return t

    t_best = np.minimum(t_best, plane([0, 1, 0], 1.3))    # floor (y down)
    t_best = np.minimum(t_best, plane([0, 0, 1], 3.6))    # back wall
    t_best = np.minimum(t_best, plane([-1, 0, 0], 2.1))   # left wall x = -2.1
    # sphere
    sc = np.array([0.35, 0.45, 2.3])
    sr = 0.55
    oc = o - sc
    a = np.einsum("ijk,ijk->ij", w, w)
    b = 2.0 * (w @ oc)
    cc = oc @ oc - sr * sr
    disc = b * b - 4 * a * cc
    with np.errstate(invalid="ignore"):
        ts = (-b - np.sqrt(disc)) / (2 * a)
    ts[~(disc > 0) | ~(ts > 1e-6)] = np.inf
    t_best = np.minimum(t_best, ts)
    if noise_sigma > 0:
        t_best = t_best + rng.normal(0.0, noise_sigma, t_best.shape)
    d = np.rint(t_best * 5000.0)
    d[~np.isfinite(d)] = 0
    d[(d < 1000) | (d > 25000)] = 0  # SLAM.cpp:229 filterDepthImage range (SLAM.hpp:15-16)
    return d.astype(np.uint16)


def kinect_pair(rows=480, cols=640, valid=0.30, seed=2, rot_deg=(0.0, 2.0, 0.0),
                shift=(0.03, 0.0, 0.0), noise_sigma=0.002, fx=FX, cx=CX, world_offset=True):
    """Config 2 / 3 / 4 workload: two depth frames of the same room, the second
    after a small camera motion, independent Bernoulli validity masks.
    Returns dict(source (3,Ns), target (3,Nt), depth_src, depth_tgt, R_true, t_true)
    where source = current frame (`data`), target = previous frame."""
    rng_t = np.random.default_rng(seed)
    rng_s = np.random.default_rng(seed + 1)
    depth_t = render_room_depth(rows, cols, np.eye(3), np.zeros(3), fx, cx, noise_sigma, rng_t)
    Rm = rot_xyz_deg(*rot_deg)
    depth_s = render_room_depth(rows, cols, Rm, np.asarray(shift, np.float64), fx, cx, noise_sigma, rng_s)
    keep_t = rng_t.random((rows, cols)) < valid
    keep_s = rng_s.random((rows, cols)) < valid
    depth_t = np.where(keep_t, depth_t, 0).astype(np.uint16)
    depth_s = np.where(keep_s, depth_s, 0).astype(np.uint16)
    tgt = backproject(depth_t, None, fx, cx)
    src = backproject(depth_s, None, fx, cx)
    if world_offset:
        tgt = tgt + CAMERA_START
        src = src + CAMERA_START
    return dict(source=src.astype(np.float32), target=tgt.astype(np.float32),
                depth_src=depth_s, depth_tgt=depth_t, R_true=Rm,
                t_true=np.asarray(shift, np.float64), fx=float(fx), cx=float(cx))


def frustum_pair(n=10000, seed=1, rot_deg=(0.0, 5.0, 0.0), shift=(0.02, -0.01, 0.03)):
    """Config 1: n points uniform in the Kinect frustum (z in [0.5, 4] m, pixel
    coordinates uniform), source = target rotated by the reference's
    makeRotationMatrix convention about the cloud centroid plus a shift."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.5, 4.0, n)
    u = rng.uniform(0, 640, n)
    v = rng.uniform(0, 480, n)
    tgt = np.stack([(u - float(CX)) * z / float(FX), (v - float(CX)) * z / float(FX), z])
    R = rot_xyz_deg(*rot_deg)
    c = tgt.mean(axis=1, keepdims=True)
    src = R @ (tgt - c) + c + np.asarray(shift, np.float64)[:, None]
    return dict(source=src.astype(np.float32), target=tgt.astype(np.float32), R_true=R,
                t_true=np.asarray(shift, np.float64))


def dense_pair(n=1_000_000, seed=5, rot_deg=(0.0, 1.0, 0.0), shift=(0.01, 0.0, 0.0)):
    """Config 5: n points on a noisy wavy surface inside a 4 x 3 x 3 m box."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2.0, 2.0, n)
    y = rng.uniform(-1.5, 1.5, n)
    z = 2.5 + 0.4 * np.sin(1.7 * x) * np.cos(2.3 * y) + rng.normal(0, 0.003, n)
    tgt = np.stack([x, y, z]) + float(CAMERA_START)
    R = rot_xyz_deg(*rot_deg)
    c = tgt.mean(axis=1, keepdims=True)
    src = R @ (tgt - c) + c + np.asarray(shift, np.float64)[:, None]
    perm = rng.permutation(n)
    return dict(source=src[:, perm].astype(np.float32), target=tgt.astype(np.float32), R_true=R,
                t_true=np.asarray(shift, np.float64))


def lattice_wall(rows=60, cols=80, z=2.0, shift_px=0.5):
    """Tie-heavy case: a flat wall sampled on the
    pixel lattice, source shifted by half a pixel so that many queries have two
    or more targets at exactly the same float distance."""
    v, u = np.mgrid[0:rows, 0:cols].astype(np.float32)
    step = np.float32(0.01)
    tgt = np.stack([(u * step).ravel(), (v * step).ravel(), np.full(rows * cols, z, np.float32)])
    src = tgt.copy()
    src[0] += np.float32(shift_px) * step
    return dict(source=src.astype(np.float32), target=tgt.astype(np.float32))


def _room_surface_coords(rows, cols, R_wc, c_w, fx, cx):
    """What render_room_depth's rays hit: (surf, su, sv) per pixel -- the surface (0 floor, 1 back wall, 2 left wall,
    3 sphere, -1 where render_room_depth has no depth) and the surface coordinates in metres on the three planes."""
    v, u = np.mgrid[0:rows, 0:cols].astype(np.float64)
    d_cam = np.stack([(u - float(cx)) / float(fx), (v - float(cx)) / float(fx), np.ones_like(u)], -1)
    w = d_cam @ np.asarray(R_wc, np.float64).T
    o = np.asarray(c_w, np.float64)
    t_best = np.full((rows, cols), np.inf)
    surf = np.full((rows, cols), -1)

    def hit(t, k):
        nonlocal t_best
        better = t < t_best
        t_best = np.where(better, t, t_best)
        surf[better] = k

    planes = [([0, 1, 0], 1.3), ([0, 0, 1], 3.6), ([-1, 0, 0], 2.1)]  # floor, back wall, left wall
    for k, (n, h) in enumerate(planes):
        n = np.asarray(n, np.float64)
        den = w @ n
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (h - o @ n) / den
        t[~(t > 1e-6)] = np.inf
        hit(t, k)
    sc = np.array([0.35, 0.45, 2.3])
    sr = 0.55
    oc = o - sc
    a = np.einsum("ijk,ijk->ij", w, w)
    b = 2.0 * (w @ oc)
    cc = oc @ oc - sr * sr
    disc = b * b - 4 * a * cc
    with np.errstate(invalid="ignore"):
        ts = (-b - np.sqrt(disc)) / (2 * a)
    ts[~(disc > 0) | ~(ts > 1e-6)] = np.inf
    hit(ts, 3)
    d = np.rint(t_best * 5000.0)
    surf[~np.isfinite(d) | (d < 1000) | (d > 25000)] = -1  # where render_room_depth has no depth
    p = o + w * np.where(np.isfinite(t_best), t_best, 0.0)[..., None]
    # surface coordinates (metres) of the three planes: floor (x, z), back wall (x, y), left wall (z, y)
    su = np.select([surf == 0, surf == 1, surf == 2], [p[..., 0], p[..., 0], p[..., 2]], 0.0)
    sv = np.select([surf == 0, surf == 1, surf == 2], [p[..., 2], p[..., 1], p[..., 1]], 0.0)
    return surf, su, sv


def render_room_color(rows, cols, R_wc, c_w, fx=FX, cx=CX, noise_sigma=0.0, rng=None, cell=0.3):
    """BGR colour frame of the room render_room_depth draws, registered to it pixel for pixel (same rays, same
    surfaces; the depth camera's pinhole).  Texture for FAST: on every plane, a lattice of `cell`-metre squares, most
    of which hold one bright rectangle on the darker plane -- isolated rectangles give L-corners (an ideal
    checkerboard's X-junctions are no FAST corners).  The sphere is plain, the background (no surface within the depth
    range) dark.  noise_sigma: Gaussian noise per channel, in grey levels.  Returns (rows, cols, 3) uint8."""
    surf, su, sv = _room_surface_coords(rows, cols, R_wc, c_w, fx, cx)
    iu = np.floor(su / cell).astype(np.int64)
    iv = np.floor(sv / cell).astype(np.int64)
    fu = su / cell - iu
    fv = sv / cell - iv
    hsh = (iu * 73856093) ^ (iv * 19349663) ^ (surf.astype(np.int64) * 83492791)
    hsh = (hsh ^ (hsh >> 13)) & 0xffff
    lo_u = 0.10 + 0.15 * ((hsh & 0xf) / 15.0)
    lo_v = 0.10 + 0.15 * (((hsh >> 4) & 0xf) / 15.0)
    hi_u = lo_u + 0.30 + 0.25 * (((hsh >> 8) & 0xf) / 15.0)
    hi_v = lo_v + 0.30 + 0.25 * (((hsh >> 12) & 0xf) / 15.0)
    rect = (surf >= 0) & (surf <= 2) & (hsh % 5 != 0) & (fu > lo_u) & (fu < hi_u) & (fv > lo_v) & (fv < hi_v)
    base = np.array([[70, 60, 50], [55, 65, 75], [60, 70, 55], [120, 130, 140]], np.float64)  # B, G, R per surface
    img = np.full((rows, cols, 3), 25.0)
    for k in range(4):
        img[surf == k] = base[k]
    tint = np.stack([(hsh & 0x3f), ((hsh >> 6) & 0x3f), ((hsh >> 10) & 0x3f)], -1).astype(np.float64)
    img = np.where(rect[..., None], 170.0 + tint, img)
    if noise_sigma > 0:
        rng = rng if rng is not None else np.random.default_rng(0)
        img = img + rng.normal(0.0, noise_sigma, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _hash8(iu, iv, surf, octave):
    """an 8-bit integer hash of the cell (iu, iv) of surface `surf` at octave `octave`"""
    h = (iu * 73856093) ^ (iv * 19349663) ^ (surf.astype(np.int64) * 83492791) ^ (octave * 2654435761)
    h = (h ^ (h >> 13)) * 1274126177
    h = h ^ (h >> 16)
    return (h & 0xff).astype(np.float64)


def render_room_textured(rows, cols, R_wc, c_w, fx=FX, cx=CX, noise_sigma=0.0, rng=None):
    """BGR colour frame of render_room_color's room under a richer texture, registered to render_room_depth in the same
    way.  On the three planes the grey value is 20 + 0.85 (0.35 h(0.32 m) + 0.35 h(0.12 m) + 0.30 h(0.045 m)), h an
    8-bit hash of the cell indices at that cell size, of the surface and of the octave: three octaves of piecewise
    constant noise, so that no two corners look alike and no large area is flat (descriptors need both; the isolated
    rectangles of render_room_color give neither).  The three channels are equal on the planes.  The sphere and the
    background are as in render_room_color.  noise_sigma: Gaussian noise per channel, in grey levels.  Returns
    (rows, cols, 3) uint8."""
    surf, su, sv = _room_surface_coords(rows, cols, R_wc, c_w, fx, cx)
    grey = np.zeros((rows, cols))
    for octave, (cell, weight) in enumerate(((0.32, 0.35), (0.12, 0.35), (0.045, 0.30))):
        iu = np.floor(su / cell).astype(np.int64)
        iv = np.floor(sv / cell).astype(np.int64)
        grey += weight * _hash8(iu, iv, surf, octave)
    grey = 20.0 + 0.85 * grey
    img = np.full((rows, cols, 3), 25.0)
    img[surf == 3] = [120, 130, 140]
    plane = (surf >= 0) & (surf <= 2)
    img[plane] = grey[plane][:, None]
    if noise_sigma > 0:
        rng = rng if rng is not None else np.random.default_rng(0)
        img = img + rng.normal(0.0, noise_sigma, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def textured_wall_pair(rows=60, cols=80, relief=0.0, seed=1, jitter=0.002, step=0.01, z=2.0, shift=(0.012, -0.008, 0.004),
                       rot_z_deg=0.5):
    """A textured wall for colored ICP: geometry that leaves the in-plane motion free, and a smooth intensity that pins
    it.  The target is a rows x cols lattice (`step` metres) at depth z, every point moved in the plane by up to
    +-jitter (uniform, from `seed`); the source samples the same wall on the lattice offset by half a step, with a
    jitter of its own, seen from a camera that has moved: source = T_true^-1 (wall points).  relief: amplitude (metres)
    of a smooth height field z += relief * (sin(2 pi x / 0.4) + cos(2 pi y / 0.3)) / 2 -- 0 is an exact plane.
    Intensity of a wall point: 0.5 + 0.25 sin(2 pi x / 0.2) + 0.2 cos(2 pi y / 0.15), in [0.05, 0.95].
    T_true: rot_z_deg about the wall's centre, then `shift`; aligning source onto target should return it.
    Returns dict(source, target (3, n) float32, source_intensity, target_intensity (n,) float32, T_true (4, 4) float64)."""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:rows, 0:cols].astype(np.float64)

    def wall(offset):
        x = (u.ravel() + offset) * step + rng.uniform(-jitter, jitter, rows * cols)
        y = (v.ravel() + offset) * step + rng.uniform(-jitter, jitter, rows * cols)
        zz = z + relief * 0.5 * (np.sin(2 * np.pi * x / 0.4) + np.cos(2 * np.pi * y / 0.3))
        inten = 0.5 + 0.25 * np.sin(2 * np.pi * x / 0.2) + 0.2 * np.cos(2 * np.pi * y / 0.15)
        return np.stack([x, y, zz]), inten

    tgt, it = wall(0.0)
    ws, is_ = wall(0.5)
    a = np.deg2rad(rot_z_deg)
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    c = np.array([0.5 * (cols - 1) * step, 0.5 * (rows - 1) * step, z])
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = c - R @ c + np.asarray(shift, np.float64)
    src = R.T @ (ws - T[:3, 3:4])
    return dict(source=src.astype(np.float32), target=tgt.astype(np.float32), source_intensity=is_.astype(np.float32),
                target_intensity=it.astype(np.float32), T_true=T)


def textured_wall_frames(poses, rows=60, cols=80, fx=60.0, cx=None, z=1.0, relief=0.0):
    """Depth and intensity frames of textured_wall_pair's wall seen through a pinhole (fx, cx for both axes, as
    everywhere here) from the given camera-to-world poses ((4, 4) each).  The wall is the surface
    z_w = z + relief * (sin(2 pi x / 0.4) + cos(2 pi y / 0.3)) / 2 of the world frame -- relief 0 is the exact plane
    z_w = z -- without a border: it covers the whole image at every pose that looks at it.  The intensity of a wall
    point is 0.5 + 0.25 sin(2 pi x / 0.2) + 0.2 cos(2 pi y / 0.15).  cx None: (cols - 1) / 2.
    Returns a list of (depth (rows, cols) uint16 at 5000 per metre, intensity (rows, cols) float32)."""
    cx = 0.5 * (cols - 1) if cx is None else cx
    v, u = np.mgrid[0:rows, 0:cols].astype(np.float64)
    ray = np.stack([(u - cx) / fx, (v - cx) / fx, np.ones_like(u)])  # camera frame, z component 1: s is the depth
    out = []
    for P in poses:
        P = np.asarray(P, np.float64).reshape(4, 4)
        d = np.einsum("ab,brc->arc", P[:3, :3], ray)
        o = P[:3, 3]
        s = (z - o[2]) / d[2]
        for _ in range(20 if relief else 0):  # fixed point on the height field: it moves the hit by relief per step at most
            x, y = o[0] + s * d[0], o[1] + s * d[1]
            s = (z + relief * 0.5 * (np.sin(2 * np.pi * x / 0.4) + np.cos(2 * np.pi * y / 0.3)) - o[2]) / d[2]
        x, y = o[0] + s * d[0], o[1] + s * d[1]
        inten = 0.5 + 0.25 * np.sin(2 * np.pi * x / 0.2) + 0.2 * np.cos(2 * np.pi * y / 0.15)
        if not ((s > 0).all() and (s * 5000.0 < 65535).all()):
            raise ValueError("a pose that does not look at the wall")
        out.append((np.rint(s * 5000.0).astype(np.uint16), inten.astype(np.float32)))
    return out
