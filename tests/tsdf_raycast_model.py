"""numpy restatement of THE RAY RULE of the TSDF volume (K20, include/icpk.h) over a tsdf_model.Volume.  numpy is used
only elementwise, in float32, one rounding per operation in the order the header writes them, so that the device and
icpk_tsdf_raycast_pixels are held against it bit for bit.  All pixels march together; the loop runs over the samples."""
import numpy as np

F = np.float32

# the reason a crossing is not listed (debug output), in the order the rule tests them
LISTED, CELL_OUT_OF_RANGE, CELL_NOT_KNOWN, CORNER_WITHOUT_GRADIENT, ZERO_LENGTH = 0, 1, 2, 3, 4


def n_samples(z_near, z_far, step):
    """rule 3: N = floor((z_far - z_near) / step) + 1, in double from the float parameters"""
    return int(np.floor((float(F(z_far)) - float(F(z_near))) / float(F(step)))) + 1


def lerp(u, v, w):
    return u + w * (v - u)


def trilerp(e, w):
    """e[z][y][x]: along x for the four (y, z) pairs, then along y, then along z"""
    c00, c10 = lerp(e[0][0][0], e[0][0][1], w[0]), lerp(e[0][1][0], e[0][1][1], w[0])
    c01, c11 = lerp(e[1][0][0], e[1][0][1], w[0]), lerp(e[1][1][0], e[1][1][1], w[0])
    return lerp(lerp(c00, c10, w[1]), lerp(c01, c11, w[1]), w[2])


def cell(vol, p):
    """rule 5 up to the weights: (in range, [i_x, i_y, i_z] (0 where out of range), [w_x, w_y, w_z])"""
    inr = np.ones(p[0].shape, bool)
    g = []
    for a in range(3):
        ga = (p[a] - vol.origin[a]) / vol.voxel - F(0.5)
        inr &= (ga >= 0) & (ga < F(vol.dims[a] - 1))
        g.append(ga)
    i = [np.where(inr, ga, 0).astype(np.int64) for ga in g]
    w = [np.where(inr, ga, 0).astype(F) - ia.astype(F) for ga, ia in zip(g, i)]
    return inr, i, w


def corners(plane, i):
    """the eight values [z][y][x] of the (dz, dy, dx) plane at the cells whose lowest corners are i = [i_x, i_y, i_z]"""
    dz, dy, dx = plane.shape
    flat, at = plane.reshape(-1), i[0] + dx * (i[1] + dy * i[2])
    return [[[flat.take(at + (x + dx * (y + dy * z))) for x in (0, 1)] for y in (0, 1)] for z in (0, 1)]


def sample(vol, ok, p):
    """SAMPLE(p) for the points p (three 1-D arrays): (known, value); the value is computed where known only"""
    inr, i, w = cell(vol, p)
    known, value = np.zeros(inr.shape, bool), np.zeros(inr.shape, F)
    sub = np.flatnonzero(inr)
    if sub.size:
        isub = [ia[sub] for ia in i]
        k = np.ones(sub.shape, bool)
        for plane in np.array(corners(ok, isub)).reshape(8, -1):
            k &= plane
        sub, isub = sub[k], [ia[k] for ia in isub]
        known[sub] = True
        value[sub] = trilerp(corners(vol.tsdf, isub), [wa[sub] for wa in w])
    return known, value


def raycast(vol, pose, shape, fx, cx, z_near, z_far, step, min_weight=1, debug=False):
    """Rules 0 - 9.  Returns dict(maps (8, rows, cols) float32: x, y, z, nx, ny, nz, depth, intensity; n_hits,
    n_no_normal); with debug also crossing (rows, cols) bool, back_face (rows, cols) bool and reason (rows, cols) int8:
    why a crossing is not listed (LISTED where it is, or where there is none).  Only the rays still marching are
    sampled: the samples sit on the lattice z_n, so what is skipped changes no bit."""
    rows, cols = shape
    P = np.asarray(pose, np.float64).reshape(4, 4)
    R, c = P[:3, :3].astype(F), P[:3, 3].astype(F)
    fx, cx, z_near, step = F(fx), F(cx), F(z_near), F(step)
    N = n_samples(z_near, z_far, step)
    if min(vol.dims) < 2:  # (never in range: no sample is known)
        out = dict(maps=np.zeros((8, rows, cols), F), n_hits=0, n_no_normal=0)
        if debug:
            out.update(crossing=np.zeros(shape, bool), back_face=np.zeros(shape, bool), reason=np.zeros(shape, np.int8))
        return out
    ok = vol.weight >= min_weight
    with np.errstate(all="ignore"):
        a = np.broadcast_to(((np.arange(cols).astype(F) - cx) / fx)[None, :], shape)
        b = np.broadcast_to(((np.arange(rows).astype(F) - cx) / fx)[:, None], shape)
        d = [((R[r, 0] * a + R[r, 1] * b) + R[r, 2]).astype(F) for r in range(3)]
        point = lambda z, at=slice(None): [c[r] + z * d[r][at] for r in range(3)]
        dflat = [dr.reshape(-1) for dr in d]
        npix = rows * cols
        live = np.arange(npix)             # the rays still marching, and their state
        have_prev = np.zeros(npix, bool)
        f_prev, z_prev = np.zeros(npix, F), np.zeros(npix, F)
        crossing, back = np.zeros(npix, bool), np.zeros(npix, bool)
        z_star = np.zeros(npix, F)
        for n in range(N):
            if not live.size:
                break
            z = F(n) * step + z_near
            known, f = sample(vol, ok, [c[r] + z * dflat[r][live] for r in range(3)])
            fp, zp = f_prev[live], z_prev[live]
            both = have_prev[live] & known
            hit = both & ~(fp < 0) & (f < 0)
            end = both & (fp < 0) & ~(f < 0)
            t = fp[hit] / (fp[hit] - f[hit])
            z_star[live[hit]] = zp[hit] + t * (z - zp[hit])
            crossing[live[hit]] = True
            back[live[end]] = True
            have_prev[live] = known
            f_prev[live[known]], z_prev[live[known]] = f[known], z
            live = live[~(hit | end)]
        crossing, back, z_star = crossing.reshape(shape), back.reshape(shape), z_star.reshape(shape)
        # rule 8 at p*
        ps = point(z_star)
        inr, i, w = cell(vol, ps)
        reason = np.zeros(shape, np.int8)
        reason[crossing & ~inr] = CELL_OUT_OF_RANGE
        known = inr.copy()
        for plane in np.array(corners(ok, i)).reshape(8, -1):
            known &= plane.reshape(shape)
        reason[crossing & inr & ~known] = CELL_NOT_KNOWN
        kk, jj, ii = i[2], i[1], i[0]
        has = np.ones(shape, bool)
        g = [[[[None, None] for _ in (0, 1)] for _ in (0, 1)] for _ in range(3)]
        for z in (0, 1):
            for y in (0, 1):
                for x in (0, 1):
                    h, gr = vol._gradient(ok, kk + z, jj + y, ii + x)
                    has &= h
                    for axis in range(3):
                        g[axis][z][y][x] = gr[axis]
        reason[crossing & known & ~has] = CORNER_WITHOUT_GRADIENT
        m = [trilerp(g[axis], w).astype(F) for axis in range(3)]
        length = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
        reason[crossing & known & has & ~(length > 0)] = ZERO_LENGTH
        listed = crossing & (reason == LISTED)
        nrm = [m[axis] / length for axis in range(3)]
        inten = trilerp(corners(vol.intensity, i), w).astype(F) if vol.intensity is not None else np.zeros(shape, F)
    maps = np.stack([np.where(listed, v, F(0)).astype(F) for v in (*ps, *nrm, z_star, inten)])
    out = dict(maps=maps, n_hits=int(listed.sum()), n_no_normal=int((crossing & ~listed).sum()))
    if debug:
        out.update(crossing=crossing, back_face=back, reason=reason)
    return out

