"""Seeded soak cases shared by tools/soak_grid.py, tools/soak_align.py, tools/soak_batch.py, tools/soak_flavours.py,
tools/soak_neighbourhoods.py (long runs, builder side) and tests/test_gpu_soak.py (a bounded slice of each inside
`-m gpu`, so that the driver runs them too).

Every case compares the product's default path (grid sweep, device loop, lock-step groups) with an independent one:
the exact kernel (literal arithmetic of icp.cpp:566-620 per pair, no spatial index) and the host loop, the same
pairs one by one, or -- the neighbourhood kernels -- the numpy model of the rule (tests/*_model.py).  Bit for bit.
soak_grid, soak_align and soak_batch return (cases_run, mismatches) and stop early after `budget_s`; soak_flavours and
soak_neighbourhoods run every case they are asked for.  Their cases come from flavour_cases / neighbourhood_cases, which
draw everything a case needs and never load the library (tests/test_soak_cases_host.py reads them without a GPU)."""
import os
import time

import numpy as np
from scipy.spatial import cKDTree

import normals_model as nm
from icp_slam_prototype_amd import binding, synth

KINDS = ["uniform", "clusters", "line", "plane_lattice", "duplicates", "tiny", "huge"]
# two more kinds for the newer slices only (len(KINDS) seeds the cases of soak_grid / soak_align / soak_batch): a plane of
# constant x -- the grid over it has nx = 1 -- and a lattice line along z -- a grid of 1 x 1 x N cells
EXTRA_KINDS = ("plane_x", "line_z")
ALL_KINDS = tuple(KINDS) + EXTRA_KINDS
LATTICE_KINDS = ("plane_lattice", "line_z")


def fuzz_cloud(rng, n, kind):
    if kind == "uniform":
        return rng.uniform(-3, 3, (3, n))
    if kind == "clusters":
        c = rng.uniform(-3, 3, (3, 12))
        return c[:, rng.integers(0, 12, n)] + rng.normal(0, 0.02, (3, n))
    if kind == "line":
        t = rng.uniform(0, 1, n)
        return np.stack([t * 4 - 2, 0.5 * t, np.full(n, 1.0)]) + rng.normal(0, 1e-4, (3, n))
    if kind == "plane_lattice":
        k = int(np.ceil(np.sqrt(n)))
        u, v = np.meshgrid(np.arange(k), np.arange(k))
        return np.stack([u.ravel()[:n] * 0.01, v.ravel()[:n] * 0.01, np.full(n, 2.0)])
    if kind == "duplicates":
        base = rng.uniform(-1, 1, (3, max(n // 7, 1)))
        return base[:, rng.integers(0, base.shape[1], n)]
    if kind == "tiny":
        return rng.uniform(-1, 1, (3, n)) * 1e-6
    return rng.uniform(-1, 1, (3, n)) * 1e4  # "huge"


def soak_grid(ctx, n_cases, seed0=5000, budget_s=None, oracle=None, log=None):
    """grid scan vs exact kernel (or the CPU oracle) over a first, unseeded sweep and two seeded ones, the source
    moving in between (icp.cpp:541-593)."""
    t0 = time.time()
    bad = done = 0
    for c in range(n_cases):
        if budget_s is not None and time.time() - t0 > budget_s:
            break
        rng = np.random.default_rng(seed0 + c)
        kt, ks = KINDS[rng.integers(0, 7)], KINDS[rng.integers(0, 7)]
        nt, nq = int(rng.integers(1, 60000)), int(rng.integers(1, 40000))
        if oracle is not None:
            nt, nq = 1 + nt // 3, 1 + nq // 3
        off = rng.uniform(-10, 10, (3, 1))
        scale = float(10.0 ** rng.uniform(-2, 1))
        tgt = (fuzz_cloud(rng, nt, kt) * scale + off).astype(np.float32)
        src = (fuzz_cloud(rng, nq, ks) * scale + off + rng.normal(0, 0.01 * scale, (3, 1))).astype(np.float32)
        if rng.random() < 0.3:
            tgt = tgt[:, rng.permutation(nt)]
        ctx.set_target(tgt)
        ctx.set_source(src)
        cur = src
        for sweep in range(3):
            if oracle is not None:
                ie, de = oracle.nn_bruteforce(cur, tgt, threads=oracle.max_threads())
            else:
                ie, de = ctx.nn(binding.NN_EXACT)
            if sweep == 0:
                ctx.reset_source()  # first grid sweep unseeded (expanding search)
            ig, dg = ctx.nn(binding.NN_GRID)
            ok = np.array_equal(ie, ig) and np.array_equal(de.view(np.uint32), dg.view(np.uint32))
            if not ok:
                bad += 1
                if log:
                    log(f"MISMATCH case {c} {kt} {ks} {nt} {nq} sweep {sweep} {int((ie != ig).sum())}")
            R = synth.rot_xyz_deg(*rng.uniform(-2, 2, 3)).astype(np.float32)
            tr = (rng.normal(0, 0.02, 3) * scale).astype(np.float32)
            ctx.transform_source(R, tr)
            if oracle is not None:
                cur = oracle.transform_points(cur, R, tr)
        done += 1
        if log and c % 20 == 19:
            log(f"{c + 1} cases, {bad} mismatches, {time.time() - t0:.0f} s")
    return done, bad


def soak_align(ctx, n_cases, seed0=9000, budget_s=None, log=None):
    """whole alignments (icp.cpp:155-258): grid scan + device loop vs exact kernel + host loop -- transform, status,
    iterations, pair count, mse, associations, moved source."""
    t0 = time.time()
    bad = done = 0
    for c in range(n_cases):
        if budget_s is not None and time.time() - t0 > budget_s:
            break
        rng = np.random.default_rng(seed0 + c)
        if rng.random() < 0.5:
            p = synth.kinect_pair(rows=int(rng.integers(40, 200)), cols=int(rng.integers(60, 260)), valid=float(rng.uniform(0.2, 1.0)),
                                  seed=int(rng.integers(0, 1 << 30)), rot_deg=tuple(rng.uniform(-3, 3, 3)),
                                  shift=tuple(rng.uniform(-0.05, 0.05, 3)))
            src, tgt = p["source"], p["target"]
        else:
            nt, nq = int(rng.integers(50, 30000)), int(rng.integers(50, 20000))
            tgt = (fuzz_cloud(rng, nt, "clusters" if rng.random() < 0.5 else "uniform") + 5).astype(np.float32)
            src = (tgt[:, rng.integers(0, nt, nq)] + rng.normal(0, 0.02, (3, nq))).astype(np.float32)
        if min(src.shape[1], tgt.shape[1]) < 10:
            continue
        solve = int(rng.integers(0, 2))
        kw = dict(solve=solve, max_iterations=int(rng.integers(1, 12)), max_nn_dist=float(rng.choice([0.75, 0.1, 0.03])))
        if rng.random() < 0.5:
            kw["fixed_iterations"] = 1
        else:
            kw["threshold"] = float(10 ** rng.uniform(-6, -3))
        res = []
        for mode, host_loop in ((binding.NN_GRID, 0), (binding.NN_EXACT, 1)):
            ctx.set_target(tgt)
            ctx.set_source(src)
            T, st, rc = ctx.align(nn_mode=mode, host_loop=host_loop, **kw)
            idx, dist = ctx.get_associations()
            res.append((T.copy(), rc, st.iterations, st.final_pairs, st.final_mse, idx, dist, ctx.get_source()))
        a, b = res
        ok = (np.array_equal(a[0], b[0]) and a[1:5] == b[1:5] and np.array_equal(a[5], b[5]) and
              np.array_equal(a[6].view(np.uint32), b[6].view(np.uint32)) and np.array_equal(a[7].view(np.uint32), b[7].view(np.uint32)))
        if not ok:
            bad += 1
            if log:
                log(f"MISMATCH case {c} {kw} {src.shape} {tgt.shape} {a[1:5]} {b[1:5]}")
        done += 1
        if log and c % 50 == 49:
            log(f"{c + 1} cases, {bad} mismatches, {time.time() - t0:.0f} s")
    return done, bad


def soak_batch(n_batches, seed0=12000, budget_s=None, device=False, log=None, groups=(1, 2, 3, 5, 8, 16)):
    """random batches through icpk_align_batch against the same pairs one by one through icpk_align: random group
    sizes, ragged pair sizes, both flavours, threshold exits, far-apart pairs (fallback), empty sources.
    Returns (pairs_run, mismatches)."""
    if device:
        import torch
    single = binding.Context(0)
    ctxs = {}
    t0 = time.time()
    bad = pairs_done = 0
    saved = os.environ.get("ICPK_BATCH_GROUP")
    try:
        for c in range(n_batches):
            if budget_s is not None and time.time() - t0 > budget_s:
                break
            rng = np.random.default_rng(seed0 + c)
            g = int(rng.choice(list(groups)))
            if g not in ctxs:
                os.environ["ICPK_BATCH_GROUP"] = str(g)
                ctxs[g] = binding.Context(0)
            ctx = ctxs[g]
            n = int(rng.integers(1, 3 * g + 2))
            pairs = []
            for k in range(n):
                u = rng.random()
                if u < 0.45:
                    p = synth.kinect_pair(rows=int(rng.integers(20, 160)), cols=int(rng.integers(30, 200)),
                                          valid=float(rng.uniform(0.2, 1.0)), seed=int(rng.integers(0, 1 << 30)),
                                          rot_deg=tuple(rng.uniform(-3, 3, 3)), shift=tuple(rng.uniform(-0.05, 0.05, 3)))
                    s, t = p["source"], p["target"]
                elif u < 0.9:
                    nt, nq = int(rng.integers(1, 20000)), int(rng.integers(1, 15000))
                    scale = float(10.0 ** rng.uniform(-2, 1))
                    off = rng.uniform(-10, 10, (3, 1))
                    t = (fuzz_cloud(rng, nt, KINDS[rng.integers(0, 7)]) * scale + off).astype(np.float32)
                    s = (fuzz_cloud(rng, nq, KINDS[rng.integers(0, 7)]) * scale + off + rng.normal(0, 0.01 * scale, (3, 1))).astype(np.float32)
                elif u < 0.95:  # far apart: < 3 pairs within reach -> fallback
                    q = synth.frustum_pair(int(rng.integers(3, 500)), seed=int(rng.integers(0, 1 << 30)))
                    s, t = q["source"] + np.float32(100), q["target"]
                else:
                    q = synth.frustum_pair(int(rng.integers(3, 500)), seed=int(rng.integers(0, 1 << 30)))
                    s, t = np.zeros((3, 0), np.float32), q["target"]
                pairs.append((np.ascontiguousarray(s, np.float32), np.ascontiguousarray(t, np.float32)))
            kw = dict(solve=int(rng.integers(0, 2)), max_iterations=int(rng.integers(0, 12)), fixed_iterations=int(rng.random() < 0.5),
                      max_nn_dist=float(rng.choice([0.75, 0.1, 0.02])), last_translation=rng.normal(0, 0.1, 3).astype(np.float32))
            if device:
                keep = [(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda()) for s, t in pairs]
                torch.cuda.synchronize()
                args = [(a.data_ptr(), a.shape[1], b_.data_ptr(), b_.shape[1]) for a, b_ in keep]
                T, st, rc = ctx.align_batch_device(args, binding.default_params(**kw))
                assoc = None
            else:
                T, st, rc, assoc = ctx.align_batch(pairs, associations=True, **kw)
            for b, (s, t) in enumerate(pairs):
                single.set_target(t)
                single.set_source(s)
                Ts, sts, rcs = single.align(**kw)
                ok = np.array_equal(T[b].view(np.uint32), Ts.view(np.uint32)) and (st[b].iterations, st[b].status, st[b].final_pairs) == (
                    sts.iterations, sts.status, sts.final_pairs)
                if s.shape[1] > 0 and assoc is not None:
                    i1, d1 = single.get_associations()
                    ok = ok and np.array_equal(assoc[b][0], i1) and np.array_equal(assoc[b][1].view(np.uint32), d1.view(np.uint32))
                if not ok:
                    bad += 1
                    if log:
                        log(f"MISMATCH batch {c} pair {b} group {g} {s.shape} {t.shape} {kw}")
                pairs_done += 1
            if log and c % 10 == 9:
                log(f"{c + 1} batches, {pairs_done} pairs, {bad} mismatches, {time.time() - t0:.0f} s")
    finally:
        if saved is None:
            os.environ.pop("ICPK_BATCH_GROUP", None)
        else:
            os.environ["ICPK_BATCH_GROUP"] = saved
        single.close()
        for cx in ctxs.values():
            cx.close()
    return pairs_done, bad


# ------------------------------------------------------------------------------------------- the newer slices: cases --
FLAVOURS = ("p2l", "robust_kabsch", "robust_p2l", "plane_to_plane", "colored")
FEATURES = ("voxel", "normals", "filters", "score", "fpfh", "color_gradients")
OUTCOMES = ("ok_fixed", "ok_threshold", "few_at_0", "few_later", "degenerate")
DEGENERATE_FLAVOURS = ("p2l", "robust_p2l", "plane_to_plane", "colored")  # the ones that solve a 6 x 6 system
RADIUS_CLASSES = ("random", "below", "above", "tie")
# points per neighbourhood case: what keeps one call of the feature's numpy model short (score and fpfh are brute force)
FEATURE_MAX_POINTS = dict(voxel=4000, normals=4000, filters=2500, score=1500, fpfh=1200, color_gradients=4000)
WHOLE_CLOUD_MAX_POINTS = 600   # ... and with a radius above the cloud's diameter
MEAN_NEIGHBOURS = 200          # ... and the mean neighbourhood a drawn radius may reach
TIE_MIN_POINTS = 600           # a lattice of at least so many points: hundreds of pairs at exactly one float32 distance
# the clouds of a context a feature is run on in EVERY case: 0 the source, 1 the target (the moments of K12 and the
# sums of K17 exist for the target alone; the source's normals are held to the target's bits)
FEATURE_SIDES = dict(voxel=(0, 1), normals=(1, 0), filters=(0, 1), score=(0, 1), fpfh=(0, 1), color_gradients=(1,))
# the slices of tests/test_gpu_soak.py: (cases, first seed)
SLICES = dict(voxel=(36, 20000), normals=(36, 21000), filters=(36, 22000), score=(36, 23000), fpfh=(36, 24000),
              color_gradients=(36, 25000),
              p2l=(120, 30000), robust_kabsch=(120, 31440), robust_p2l=(120, 32000), plane_to_plane=(120, 33300),
              colored=(120, 34000))


def any_cloud(rng, n, kind):
    if kind == "plane_x":
        return np.stack([np.full(n, 1.0), rng.uniform(-2, 2, n), rng.uniform(-2, 2, n)])
    if kind == "line_z":
        return np.stack([np.full(n, 0.5), np.full(n, -0.25), np.arange(n) * 0.01])
    return fuzz_cloud(rng, n, kind)


def distinct_finite(pts):
    """the distinct finite points of a (3, n) float32 cloud, (3, k)"""
    p = pts[:, np.isfinite(pts).all(0)]
    return np.unique(p, axis=1) if p.shape[1] else p


def cloud_geometry(pts):
    """dict(spacing: the median distance of a distinct point to its nearest other one, smallest: the least such
    distance, diameter: the bounding box's diagonal, tie: the float32 nearest-neighbour distance (icp.cpp:606-620) that
    most points share, distinct: how many distinct finite points there are).  A cloud of fewer than two distinct points
    has no spacing: a thousandth of its largest coordinate (or of 1) stands in."""
    u = distinct_finite(pts)
    k = u.shape[1]
    if k < 2:
        s = 1e-3 * max(float(np.abs(u).max(initial=0.0)), 1.0)
        return dict(spacing=s, smallest=s, diameter=0.0, tie=float(np.float32(s)), distinct=k)
    d, j = cKDTree(u.astype(np.float64).T).query(u.astype(np.float64).T, k=2)
    vals, counts = np.unique(nm.pair_dist(u, u[:, j[:, 1]]).astype(np.float32), return_counts=True)
    box = u.astype(np.float64)
    return dict(spacing=float(np.median(d[:, 1])), smallest=float(d[:, 1].min()),
                diameter=float(np.linalg.norm(box.max(1) - box.min(1))), tie=float(vals[np.argmax(counts)]), distinct=k)


def _capped(pts, r):
    """r, shrunk until a neighbourhood holds at most MEAN_NEIGHBOURS points on average (over a sample of the cloud)"""
    p = pts[:, np.isfinite(pts).all(0)].astype(np.float64).T
    if len(p) < 2:
        return r
    tree = cKDTree(p)
    sample = p[::max(1, len(p) // 128)]
    for _ in range(40):
        if tree.query_ball_point(sample, r, return_length=True).mean() <= MEAN_NEIGHBOURS:
            break
        r *= 0.7
    return r


def _radius(rng, pts, geo, rclass):
    """the radius (leaf, max_dist) of a class, as the float32 the library will read"""
    if rclass == "below":
        r = 0.5 * geo["smallest"]
    elif rclass == "above":
        r = 2.0 * geo["diameter"] if geo["diameter"] > 0 else 4.0 * geo["spacing"]
    elif rclass == "tie":
        r = geo["tie"]
    else:
        r = _capped(pts, geo["spacing"] * float(np.exp(rng.uniform(np.log(0.5), np.log(8.0)))))
    return float(np.float32(r))


def _sprinkle(rng, pts):
    """exact duplicates (1 %) and non-finite points (0.5 %), in place"""
    n = pts.shape[1]
    if n < 8:
        return
    k = max(1, n // 100)
    pts[:, rng.integers(0, n, k)] = pts[:, rng.integers(0, n, k)]
    bad = rng.integers(0, n, max(1, n // 200))
    pts[rng.integers(0, 3, bad.size), bad] = rng.choice(np.float32([np.nan, np.inf, -np.inf]), bad.size)


def _unit(rng, k, zero_share=0.0):
    v = rng.normal(size=(3, k))
    v = (v / np.linalg.norm(v, axis=0)).astype(np.float32)
    v[:, rng.random(k) < zero_share] = 0
    return v


def _log_int(rng, lo, hi):
    return int(round(10.0 ** rng.uniform(np.log10(lo), np.log10(hi))))


def _perturbed(rng, tgt, nq, sigma):
    """nq points of tgt, moved by N(0, sigma) (sigma 0: the same bits)"""
    pick = tgt[:, rng.integers(0, tgt.shape[1], nq)]
    if sigma == 0:
        return pick.copy()
    return (pick.astype(np.float64) + rng.normal(0, sigma, (3, nq))).astype(np.float32)


def _pose(rng, centre, rot_deg, shift):
    """row-major 4 x 4 float32: a rotation about `centre`, then a shift"""
    R = synth.rot_xyz_deg(*rng.uniform(-rot_deg, rot_deg, 3))
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = centre - R @ centre + rng.normal(0, 1, 3) * shift
    return T.astype(np.float32)


def neighbourhood_cases(feature, n_cases, seed0):
    """The cases of soak_neighbourhoods: case c is of kind ALL_KINDS[c % 9] and radius class RADIUS_CLASSES[c % 4]
    (`tie` on the lattice kinds only, elsewhere another drawn radius), so that 36 cases in a row hold every combination
    and nine hold every kind and every class.  A case is a dict of numpy arrays and numbers; `r` is the radius, leaf or
    max_dist.  On every other round the `tiny` kind takes the smallest scale, where an offset of order 10 rounds the
    whole cloud to one repeated float32 point."""
    assert feature in FEATURES
    for c in range(n_cases):
        rng = np.random.default_rng(seed0 + c)
        kind = ALL_KINDS[c % len(ALL_KINDS)]
        rclass = RADIUS_CLASSES[c % 4]
        if rclass == "tie" and kind not in LATTICE_KINDS:
            rclass = "random"
        n = _log_int(rng, 5, FEATURE_MAX_POINTS[feature])
        if rclass == "above":
            n = min(n, WHOLE_CLOUD_MAX_POINTS)
        if rclass == "tie":
            n = max(n, TIE_MIN_POINTS)
        off = rng.uniform(-10, 10, (3, 1))
        e = rng.uniform(-2, 1)
        if kind == "tiny" and (c // len(ALL_KINDS)) % 2 == 0:
            e = -2.0
        scale = float(10.0 ** e)
        pts = (any_cloud(rng, n, kind) * scale + off).astype(np.float32)
        _sprinkle(rng, pts)
        geo = cloud_geometry(pts)
        r = _radius(rng, pts, geo, rclass)
        case = dict(name=f"{feature} seed {seed0 + c} {kind} n {n} r {rclass} {r:.9g}", feature=feature, kind=kind,
                    rclass=rclass, pts=pts, r=r, scale=scale, distinct=geo["distinct"])
        if feature == "voxel":
            case["normals"] = (rng.normal(0, 1, (3, n)) * (rng.random(n) > 0.1)).astype(np.float32)
        elif feature == "normals":
            case["min_neighbors"] = int(rng.integers(3, 10))
            case["viewpoint"] = None if rng.random() < 0.3 else (off[:, 0] + rng.normal(0, 3 * scale, 3)).astype(np.float32)
        elif feature == "filters":
            case.update(k=int(rng.integers(1, binding.FILTER_MAX_K + 1)), std_ratio=float(rng.uniform(0.3, 3.0)),
                        min_neighbors=int(rng.integers(1, 12)))
        elif feature == "score":
            nq = _log_int(rng, 5, FEATURE_MAX_POINTS[feature])
            sigma = 0.0 if rng.random() < 1 / 6 else r * float(rng.uniform(0.05, 1.0))
            src = _perturbed(rng, pts, nq, sigma)
            far = rng.random(nq) < 0.1
            src[:, far] += np.float32(3 * max(geo["diameter"], geo["spacing"]))
            centre = np.nan_to_num(pts.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0).mean(1)
            poses = [np.eye(4, dtype=np.float32), _pose(rng, centre, 2.0, 0.5 * r), _pose(rng, centre, 0.2, 0.1 * r),
                     _pose(rng, centre, 2.0, 0.5 * r), _pose(rng, centre, 40.0, 10 * max(geo["diameter"], r))]
            poses[3][int(rng.integers(0, 3)), int(rng.integers(0, 4))] = rng.choice(np.float32([np.nan, np.inf]))
            case.update(source=src, poses=np.stack(poses), zero_noise=sigma == 0.0)
        elif feature == "fpfh":
            nq = _log_int(rng, 5, FEATURE_MAX_POINTS[feature])
            if rclass == "above":
                nq = min(nq, WHOLE_CLOUD_MAX_POINTS)
            sigma = 0.0 if rng.random() < 1 / 6 else geo["spacing"] * float(rng.uniform(0.05, 1.0))
            tn, sn = _unit(rng, n, 0.1), _unit(rng, nq, 0.1)
            for v in (tn, sn):
                if v.shape[1] >= 8:
                    v[int(rng.integers(0, 3)), int(rng.integers(0, v.shape[1]))] = np.nan
                    v[:, int(rng.integers(0, v.shape[1]))] *= np.float32(3)
            case.update(source=_perturbed(rng, pts, nq, sigma), normals=tn, source_normals=sn, zero_noise=sigma == 0.0)
        else:  # color_gradients
            nrm = _unit(rng, n, 0.1)
            inten = rng.uniform(0, 1, n).astype(np.float32)
            if n >= 8:
                nrm[:, 1] *= np.float32(3)
                nrm[0, 2] = np.nan
                nrm[:, 3] *= np.float32(1.0002)  # inside the band of usable lengths
                inten[0], inten[4] = 0.0, 1.0
            case.update(normals=nrm, intensity=inten, min_neighbors=int(rng.integers(1, 9)))
        yield case


def _accepted_estimate(src, tgt, max_dist, normals=None):
    """about how many queries the first sweep accepts: a partner within max_dist and, given uploaded target normals, one
    with a normal (a k-d tree in float64: a guide for min_pairs, nothing exact)"""
    d, j = cKDTree(tgt.astype(np.float64).T).query(src.astype(np.float64).T)
    ok = d < max_dist
    if normals is not None:
        ok &= (normals[:, j] != 0).any(0)
    return int(ok.sum())


def flavour_cases(flavour, n_cases, seed0):
    """The cases of soak_flavours: a pair of 50 ... 20 000 points a side (half of them a small depth-camera pair, half a
    cloud of a random kind, offset and scale with a source of target points plus noise, the noise exactly 0 in one case
    of six), what the flavour needs on top (normals estimated on the device or uploaded with a share of zero ones,
    intensities) and the settings of the alignment."""
    assert flavour in FLAVOURS
    robust = flavour.startswith("robust")
    reads_normals = flavour != "robust_kabsch"
    for c in range(n_cases):
        rng = np.random.default_rng(seed0 + c)
        zero_noise = bool(rng.random() < 1 / 6)
        if rng.random() < 0.5:
            kind, scale = "kinect", 1.0
            p = synth.kinect_pair(rows=int(rng.integers(20, 110)), cols=int(rng.integers(30, 170)), valid=float(rng.uniform(0.3, 1.0)),
                                  seed=int(rng.integers(0, 1 << 30)), rot_deg=tuple(rng.uniform(-3, 3, 3)),
                                  shift=tuple(rng.uniform(-0.05, 0.05, 3)))
            tgt = p["target"]
            src = _perturbed(rng, tgt, p["source"].shape[1], 0.0) if zero_noise else p["source"]
        else:
            kind = ALL_KINDS[rng.integers(0, len(ALL_KINDS))]
            nt, nq = _log_int(rng, 50, 20000), _log_int(rng, 50, 20000)
            scale = float(10.0 ** rng.uniform(-2, 1))
            off = rng.uniform(-10, 10, (3, 1))
            tgt = (any_cloud(rng, nt, kind) * scale + off).astype(np.float32)
            src = _perturbed(rng, tgt, nq, 0.0 if zero_noise else 0.02 * scale)
        nq, nt = src.shape[1], tgt.shape[1]
        kw = dict(max_iterations=int(rng.integers(1, 13)), max_nn_dist=float(rng.choice([0.75, 0.1, 0.03])) * scale)
        if rng.random() < 0.5:
            kw["fixed_iterations"] = 1
        else:
            kw["fixed_iterations"] = 0
            kw["threshold"] = float(10 ** rng.uniform(-6, -3))
        kw["last_rotation"] = synth.rot_xyz_deg(*rng.uniform(-2, 2, 3)).astype(np.float32)
        kw["last_translation"] = (rng.normal(0, 0.02, 3) * scale).astype(np.float32)
        case = dict(flavour=flavour, kind=kind, source=src, target=tgt, scale=scale, zero_noise=zero_noise, zero_normals=False)
        if reads_normals:
            sides = ("target", "source") if flavour == "plane_to_plane" else ("target",)
            if rng.random() < 0.5:
                case["normals"] = "estimated"
                for side, cloud in zip(sides, (tgt, src)):
                    case[side + "_normals"] = dict(radius=float(np.float32(cloud_geometry(cloud)["spacing"] * rng.uniform(1.5, 6.0))),
                                                   min_neighbors=int(rng.integers(3, 9)),
                                                   viewpoint=None if rng.random() < 0.5 else rng.uniform(-10, 10, 3).astype(np.float32))
            else:
                case["normals"] = "uploaded"
                share = 1.0 if rng.random() < 0.05 else float(rng.uniform(0, 0.5))
                for side, cloud in zip(sides, (tgt, src)):
                    case[side + "_normals"] = _unit(rng, cloud.shape[1], share)
                    case["zero_normals"] |= bool((case[side + "_normals"] == 0).all(0).any())
        if flavour == "colored":
            case.update(target_intensity=rng.uniform(0, 1, nt).astype(np.float32), source_intensity=rng.uniform(0, 1, nq).astype(np.float32),
                        gradient_radius=float(np.float32(cloud_geometry(tgt)["spacing"] * rng.uniform(2.0, 6.0))),
                        gradient_min_neighbors=int(rng.integers(1, 9)), lambda_geometric=float(rng.choice([0.0, 0.5, 0.968, 1.0])))
        if flavour == "plane_to_plane":
            case["epsilon"] = float(rng.choice([1e-3, 1e-2, 1.0]))
        if robust:
            kernel = int(rng.integers(0, 3))
            mode = int(rng.integers(0, 2))
            s = float(rng.choice([1.0, 2.0, 4.685])) if mode == binding.SCALE_MEDIAN else float(10 ** rng.uniform(-2.5, -0.5)) * scale
            case["robust"] = dict(kernel=kernel, scale_mode=mode, scale=s, trim=float(rng.choice([1.0, 0.8, 0.5, 1e-6])))
        # min_pairs: the default; from 0.1 % to 16 % below what the first sweep should keep (a later sweep may fall under
        # it); a share of the query count; more than the query count
        u = rng.random()
        if u < 0.6:
            kw["min_pairs"] = 3
        elif u < 0.75:
            tn = case.get("target_normals")
            n0 = _accepted_estimate(src, tgt, kw["max_nn_dist"], tn if isinstance(tn, np.ndarray) else None)
            if robust:
                n0 = int(np.ceil(case["robust"]["trim"] * n0))
            kw["min_pairs"] = max(3, int(n0 * (1.0 - 10.0 ** rng.uniform(-3, -0.8))))
        elif u < 0.9:
            kw["min_pairs"] = max(3, int(nq * rng.uniform(0.25, 1.0)))
        else:
            kw["min_pairs"] = nq + int(rng.integers(1, 10))
        case["settings"] = kw
        case["name"] = (f"{flavour} seed {seed0 + c} {kind} {nq} x {nt} iterations {kw['max_iterations']} "
                        f"{'fixed' if kw['fixed_iterations'] else 'threshold'} min_pairs {kw['min_pairs']}")
        yield case


def case_bytes(case):
    """everything a case holds, as bytes (two passes over a generator must give the same)"""
    out = []
    for k in sorted(case):
        v = case[k]
        if isinstance(v, dict):
            out.append(k.encode() + b"{" + case_bytes(v) + b"}")
        elif isinstance(v, np.ndarray):
            out.append(k.encode() + str(v.dtype).encode() + str(v.shape).encode() + np.ascontiguousarray(v).tobytes())
        else:
            out.append(k.encode() + repr(v).encode())
    return b"|".join(out)


# ---------------------------------------------------------------------------------------- the newer slices: the runs --
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def first_difference(a, b):
    """a, b: lists of (field, values).  None, or (field, index) of the first entry that differs (index -1: the sizes)"""
    if len(a) != len(b):
        return "fields", -1
    for (na, xa), (nb, xb) in zip(a, b):
        xa, xb = np.asarray(xa).reshape(-1), np.asarray(xb).reshape(-1)
        if na != nb or xa.shape != xb.shape:
            return na, -1
        bad = np.flatnonzero(xa != xb)
        if bad.size:
            return na, int(bad[0])
    return None


def _alignment(ctx, robust, **kw):
    """one alignment and everything observable it leaves, as (field, values) of integers"""
    try:
        T, st, rc = ctx.align(**kw)
        idx, dist = ctx.get_associations()
        src = ctx.get_source()
        trace = ctx.get_trace()
        rtrace = ctx.get_robust_trace() if robust else []
    except binding.IcpkError as e:
        return [("error", [e.code])], None
    f = [("rc", [rc]), ("iterations", [st.iterations]), ("status", [st.status]), ("final_pairs", [st.final_pairs]),
         ("final_mse", _bits(np.float32([st.final_mse]))), ("T", _bits(T)), ("assoc_index", idx), ("assoc_dist", _bits(dist)),
         ("source", _bits(src)), ("trace_length", [len(trace)])]
    if trace:
        f += [("trace_R", _bits(np.stack([t["R"] for t in trace]))), ("trace_t", _bits(np.stack([t["t"] for t in trace]))),
              ("trace_n_pairs", [t["n_pairs"] for t in trace]), ("trace_mse", _bits(np.float32([t["mse"] for t in trace])))]
    if robust:
        f += [("robust_trace_length", [len(rtrace)]), ("robust_kept", [t["kept"] for t in rtrace]),
              ("robust_cut", _bits(np.float32([t["cut"] for t in rtrace]))), ("robust_c", _bits(np.float64([t["c"] for t in rtrace]))),
              ("robust_wsum", _bits(np.float64([t["wsum"] for t in rtrace])))]
    return f, (rc, st.iterations)


def _outcome(rc, iterations, settings):
    if rc == binding.W_DEGENERATE:
        return "degenerate"
    if rc == binding.W_TOO_FEW_PAIRS:
        return "few_at_0" if iterations == 0 else "few_later"
    if rc != binding.OK:
        return f"status {rc}"
    if settings["fixed_iterations"]:
        return "ok_fixed" if iterations == settings["max_iterations"] else "ok_fixed_short"
    return "ok_threshold" if iterations < settings["max_iterations"] else "ok_max_iterations"


def _install_normals(ctx, case, side):
    v = case[side + "_normals"]
    if isinstance(v, dict):
        (ctx.estimate_target_normals if side == "target" else ctx.estimate_source_normals)(v["radius"], v["min_neighbors"], v["viewpoint"])
    else:
        (ctx.set_target_normals if side == "target" else ctx.set_source_normals)(v)


def run_flavour_case(ctx, case):
    """(first difference or None, outcome) of one case: the target and what goes with it are installed once; the source
    is uploaded, and what is attached to it re-attached, before each of the two runs"""
    flavour, kw = case["flavour"], case["settings"]
    robust = "robust" in case
    solve = {"robust_kabsch": binding.SOLVE_KABSCH, "plane_to_plane": binding.SOLVE_PLANE_TO_PLANE}.get(flavour, binding.SOLVE_POINT_TO_PLANE)
    try:
        ctx.set_robust(None)
        ctx.set_colored(False)
        ctx.set_target(case["target"])
        ctx.set_source(case["source"])
        attached = {}
        try:
            if "target_normals" in case:
                _install_normals(ctx, case, "target")
            if "source_normals" in case:
                _install_normals(ctx, case, "source")
                attached["normals"] = ctx.get_source_normals()
            if flavour == "colored":
                ctx.set_target_colors(case["target_intensity"])
                ctx.estimate_target_color_gradients(case["gradient_radius"], case["gradient_min_neighbors"])
                ctx.set_source_colors(case["source_intensity"])
                attached["colors"] = ctx.get_source_colors()
                ctx.set_colored(True, case["lambda_geometric"])
            if flavour == "plane_to_plane":
                ctx.set_plane_to_plane(case["epsilon"])
            if robust:
                ctx.set_robust(**case["robust"])
        except binding.IcpkError as e:
            return ("setup error", e.code), "error"
        res = []
        for mode, host_loop in ((binding.NN_GRID, 0), (binding.NN_EXACT, 1)):
            ctx.set_source(case["source"])
            if "normals" in attached:
                ctx.set_source_normals(attached["normals"])
            if "colors" in attached:
                ctx.set_source_colors(attached["colors"])
            res.append(_alignment(ctx, robust, solve=solve, nn_mode=mode, host_loop=host_loop, **kw))
        (a, ka), (b, _) = res
        return first_difference(a, b), ("error" if ka is None else _outcome(*ka, kw))
    finally:
        ctx.set_robust(None)
        ctx.set_colored(False)
        ctx.set_plane_to_plane(1e-3)


def soak_flavours(ctx, flavour, n_cases, seed0, log=None):
    """whole alignments of a newer flavour: grid scan + device loop vs exact kernel + host loop on one context --
    transform, status, iterations, pair count, mse, associations, moved source, trace, robust trace.  A warning code is a
    result like any other.  Returns (cases_run, mismatches, tally of the outcomes)."""
    t0 = time.time()
    bad = done = 0
    tally = {k: 0 for k in OUTCOMES}
    for c, case in enumerate(flavour_cases(flavour, n_cases, seed0)):
        diff, outcome = run_flavour_case(ctx, case)
        tally[outcome] = tally.get(outcome, 0) + 1
        if diff is not None or outcome == "error":
            bad += 1
            if log:
                log(f"MISMATCH {case['name']} ({outcome}): first difference in {diff[0] if diff else 'neither'} at index {diff[1] if diff else -1}")
        done += 1
        if log and c % 50 == 49:
            log(f"{c + 1} cases, {bad} mismatches, {time.time() - t0:.0f} s, {tally}")
    return done, bad, tally


def _compare(pairs):
    """pairs: (field, got, want) arrays.  None, or 'field at index' of the first entry whose bits differ"""
    d = first_difference([(f, _as_words(g)) for f, g, _ in pairs], [(f, _as_words(w)) for f, _, w in pairs])
    return None if d is None else f"{d[0]} at index {d[1]}"


def _as_words(a):
    a = np.ascontiguousarray(a)
    return _bits(a) if a.dtype.kind == "f" else a.reshape(-1)


def _nb_voxel(ctx, case):
    import voxel_model as vm

    pts, leaf = case["pts"], case["r"]
    for mode in (binding.VOXEL_FIRST, binding.VOXEL_CENTROID):
        for which, nrm in [(w, None) for w in FEATURE_SIDES["voxel"]] + [(1, case["normals"])]:
            want = vm.downsample(pts, leaf, mode, nrm)
            if which == 0:
                ctx.set_source(pts)
            else:
                ctx.set_target(pts)
                if nrm is not None:
                    ctx.set_target_normals(nrm)
            n_out, n_dropped = ctx.voxel_downsample(which, leaf, mode)
            g = ctx.get_voxel_groups()
            got = dict(points=ctx.get_source() if which == 0 else ctx.get_target(),
                       normals=ctx.get_target_normals() if nrm is not None else None, first_index=g["first_index"],
                       count=g["count"], out_of_point=g["out_of_point"], n_out=n_out, n_dropped=n_dropped)
            diff = vm.same(want, got)
            if diff is None and g["n_out"] != n_out:
                diff = "n_out of the groups"
            if diff is not None:
                return f"mode {mode} which {which} normals {nrm is not None}: {diff}"
    return None


def _nb_normals(ctx, case):
    pts, r = case["pts"], case["r"]
    want = nm.estimate(pts, r, case["min_neighbors"], case["viewpoint"])
    ctx.set_target(pts)
    ctx.estimate_target_normals(r, case["min_neighbors"], case["viewpoint"], keep_moments=True)
    st = ctx.get_normal_stats()
    diff = _compare([("n", [st["n"]], [pts.shape[1]]), ("count", st["count"], want["count"]), ("moments", st["moments"], want["moments"])])
    if diff is None and 0 in FEATURE_SIDES["normals"]:  # the source's estimate is the same rule: the target's bits
        ctx.set_source(pts)
        ctx.estimate_source_normals(r, case["min_neighbors"], case["viewpoint"])
        diff = _compare([("source normals", ctx.get_source_normals(), ctx.get_target_normals())])
    return diff


def _nb_filters(ctx, case):
    import filter_model as fm

    pts = case["pts"]
    for kind, kw in ((binding.FILTER_STATISTICAL, dict(k=case["k"], std_ratio=case["std_ratio"])),
                     (binding.FILTER_RADIUS, dict(radius=case["r"], min_neighbors=case["min_neighbors"]))):
        want = fm.remove_outliers(pts, kind, **kw)
        for which in FEATURE_SIDES["filters"]:
            (ctx.set_source if which == 0 else ctx.set_target)(pts)
            n_out, n_dropped = ctx.remove_outliers(which, kind=kind, **kw)
            got = ctx.outlier_stats()
            got.update(n_dropped=n_dropped, keep=got["out_index"] >= 0, points=ctx.get_source() if which == 0 else ctx.get_target())
            diff = fm.same(want, got)
            if diff is None and (got["n_out"] != n_out or got["n_in"] != pts.shape[1]):
                diff = "n_out / n_in of the statistics"
            if diff is not None:
                bad = -1
                if diff in want and want[diff] is not None and np.shape(want[diff]) == np.shape(got[diff]):
                    bad = int(np.flatnonzero(_as_words(want[diff]) != _as_words(got[diff]))[0])
                return f"kind {kind} which {which}: {diff} at index {bad}"
    return None


def _nb_score(ctx, case):
    import score_model as sm

    src, tgt, T, max_dist = case["source"], case["pts"], case["poses"], case["r"]
    ctx.set_target(tgt)
    ctx.set_source(src)
    out = ctx.score_poses(T, max_dist, keep_assoc=True)
    for k in range(len(T)):
        want = sm.score(src, tgt, T[k], max_dist)
        idx, dist = ctx.score_associations(k)
        diff = _compare([("inliers", [out["inliers"][k]], [want["inliers"]]), ("partner", idx, want["idx"]),
                         ("distance", dist, want["dist"]), ("sums", out["sums"][k], want["sums"])])
        if diff is not None:
            return f"pose {k}: {diff}"
    return None


def _nb_fpfh(ctx, case):
    import fpfh_model as fm

    r = case["r"]
    ctx.set_target(case["pts"])
    ctx.set_target_normals(case["normals"])
    ctx.set_source(case["source"])
    ctx.set_source_normals(case["source_normals"])
    desc = {}
    for which, pts, nrm in ((0, case["source"], case["source_normals"]), (1, case["pts"], case["normals"])):
        want = fm.fpfh(pts, nrm, r)
        ctx.compute_fpfh(which, r, keep_spfh=True)
        d, valid = ctx.get_fpfh(which)
        counts, m = ctx.get_spfh(which)
        diff = _compare([("m", m, want["m"]), ("counts", counts, want["counts"]), ("valid", valid, want["valid"]),
                         ("descriptor", d, want["desc"])])
        if diff is not None:
            return f"which {which}: {diff}"
        desc[which] = (d, valid)
    for mutual in (False, True):
        want = fm.match(desc[0][0], desc[0][1], desc[1][0], desc[1][1], mutual=mutual)
        got = ctx.match_features(mutual=mutual)
        diff = _compare([("pairs", [len(got[0])], [len(want[0])]), ("source index", got[0], want[0]),
                         ("target index", got[1], want[1]), ("D", got[2], want[2])])
        if diff is not None:
            return f"match mutual {mutual}: {diff}"
    return None


def _nb_color_gradients(ctx, case):
    import color_model as cm

    want = cm.gradient_sums(case["pts"], case["normals"], case["intensity"], case["r"])
    ctx.set_target(case["pts"])
    ctx.set_target_normals(case["normals"])
    ctx.set_target_colors(case["intensity"])
    ctx.estimate_target_color_gradients(case["r"], case["min_neighbors"], keep_sums=True)
    return _compare([("sums", ctx.color_gradient_sums(), want)])


_NB_RUN = dict(voxel=_nb_voxel, normals=_nb_normals, filters=_nb_filters, score=_nb_score, fpfh=_nb_fpfh,
               color_gradients=_nb_color_gradients)


def run_neighbourhood_model(case):
    """the numpy model of a case alone, with its own asserts (tests/test_soak_cases_host.py: the cases are ones the
    models take)"""
    import color_model as cm
    import filter_model as fm
    import fpfh_model as pm
    import score_model as sm
    import voxel_model as vm

    f, pts, r = case["feature"], case["pts"], case["r"]
    if f == "voxel":
        return [vm.downsample(pts, r, mode, nrm) for mode in (vm.FIRST, vm.CENTROID) for nrm in (None, case["normals"])]
    if f == "normals":
        return nm.estimate(pts, r, case["min_neighbors"], case["viewpoint"])
    if f == "filters":
        return [fm.remove_outliers(pts, fm.STATISTICAL, k=case["k"], std_ratio=case["std_ratio"]),
                fm.remove_outliers(pts, fm.RADIUS, radius=r, min_neighbors=case["min_neighbors"])]
    if f == "score":
        return [sm.score(case["source"], pts, T, r) for T in case["poses"]]
    if f == "fpfh":
        s, t = pm.fpfh(case["source"], case["source_normals"], r), pm.fpfh(pts, case["normals"], r)
        return [s, t] + [pm.match(s["desc"], s["valid"], t["desc"], t["valid"], mutual=m) for m in (False, True)]
    return cm.gradient_sums(pts, case["normals"], case["intensity"], r)


def soak_neighbourhoods(ctx, feature, n_cases, seed0, log=None):
    """a neighbourhood kernel (the ones that share csrc/grid_walk.h's cube walk, and the voxel grid) against the numpy
    model of its rule, bit for bit, through the feature's own comparison.  Returns (cases_run, mismatches)."""
    t0 = time.time()
    bad = done = 0
    for c, case in enumerate(neighbourhood_cases(feature, n_cases, seed0)):
        try:
            diff = _NB_RUN[feature](ctx, case)
        except binding.IcpkError as e:
            diff = f"the library refused: {e}"
        if diff is not None:
            bad += 1
            if log:
                log(f"MISMATCH {case['name']}: first difference in {diff}")
        done += 1
        if log and c % 20 == 19:
            log(f"{c + 1} cases, {bad} mismatches, {time.time() - t0:.0f} s")
    return done, bad
