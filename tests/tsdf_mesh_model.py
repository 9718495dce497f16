"""numpy restatement of the mesh rule of the TSDF volume (K21, include/icpk.h) over tsdf_model.Volume: marching
tetrahedra over the Kuhn split of every known cell.  numpy is used only elementwise, in float32, one rounding per
operation in the order the header writes them, so that the device and icpk_tsdf_mesh_host are held against it bit for
bit.  The triangle table is NOT copied from the header: it is built here from the general rule the header states behind
it (TABLE below), and tests/test_tsdf_mesh_host.py holds the two against each other through the library's bytes."""
import itertools

import numpy as np

F = np.float32

# rule 2: the tetrahedra in lexicographic order of the axis permutation (a, b, c): corners 0, 1 << a, that | 1 << b, 7
PERMS = list(itertools.permutations(range(3)))
TETS = [(0, 1 << a, (1 << a) | (1 << b), 7) for a, b, _ in PERMS]
ODD = [sum(1 for x in range(3) for y in range(x + 1, 3) if p[x] > p[y]) % 2 == 1 for p in PERMS]


def _case_triangles(case):
    """The triangles of an even tetrahedron: tuples of three (p, q) position pairs, p the position named first."""
    inside = [n for n in range(4) if (case >> n) & 1]
    outside = [n for n in range(4) if not (case >> n) & 1]
    if len(inside) in (0, 4):
        return []
    if len(inside) == 2:
        (p, q), (r, s) = inside, outside
        tris = [((p, r), (p, s), (q, s)), ((p, r), (q, s), (q, r))]
        swap = (p + q) % 2 == 0
    else:
        lone_outside = len(outside) == 1
        p = outside[0] if lone_outside else inside[0]
        tris = [tuple((p, o) for o in range(4) if o != p)]
        swap = (p % 2 == 1) != lone_outside
    return [(t[0], t[2], t[1]) if swap else t for t in tris]


TABLE = [_case_triangles(case) for case in range(16)]


def mesh(vol, min_weight=1):
    """The mesh rule.  Returns dict(vertices (3, n), normals (3, n), intensity, voxel_index int32, edge uint8, triangles
    (m, 3) int32, n_vertices, n_triangles, n_no_normal)."""
    dx, dy, dz = vol.dims
    f = vol.tsdf
    ok = vol.weight >= min_weight
    neg = f < 0
    # rule 1: known[k, j, i] for every voxel: it is the lower corner of a cell in range all of whose corners are ok
    known = np.zeros((dz, dy, dx), bool)
    if min(dx, dy, dz) >= 2:
        cell = np.ones((dz - 1, dy - 1, dx - 1), bool)
        for e in range(8):
            cell &= ok[(e >> 2) & 1:dz - 1 + ((e >> 2) & 1), (e >> 1) & 1:dy - 1 + ((e >> 1) & 1), (e & 1):dx - 1 + (e & 1)]
        known[:dz - 1, :dy - 1, :dx - 1] = cell

    def known_below(u):
        """known[V - u] per voxel V (False where V - u is out of range)"""
        out = np.zeros_like(known)
        uz, uy, ux = (u >> 2) & 1, (u >> 1) & 1, u & 1
        out[uz:, uy:, ux:] = known[:dz - uz, :dy - uy, :dx - ux]
        return out

    centres = vol.centres()
    rec = {k: [] for k in ("key", "x", "y", "z", "nx", "ny", "nz", "c", "has")}
    for m in range(1, 8):  # rule 3, one edge type at a time
        mz, my, mx = (m >> 2) & 1, (m >> 1) & 1, m & 1
        if dz - mz < 1 or dy - my < 1 or dx - mx < 1:
            continue
        sv = (slice(0, dz - mz), slice(0, dy - my), slice(0, dx - mx))
        sn = (slice(mz, dz), slice(my, dy), slice(mx, dx))
        cross = neg[sv] != neg[sn]
        contained = np.zeros_like(known)
        for u in range(8):
            if u & m == 0:
                contained |= known_below(u)
        k, j, i = np.nonzero(cross & contained[sv])
        kn, jn, in_ = k + mz, j + my, i + mx
        fv, fn = f[k, j, i], f[kn, jn, in_]
        with np.errstate(all="ignore"):
            t = fv / (fv - fn)
            step = t * vol.voxel
            hv, gv = vol._gradient(ok, k, j, i)
            hn, gn = vol._gradient(ok, kn, jn, in_)
            g = [gv[a] + t * (gn[a] - gv[a]) for a in range(3)]
            length = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
            has = hv & hn & (length > 0)
            n = [np.where(has, g[a] / length, F(0)).astype(F) for a in range(3)]
            p = [centres[0][i], centres[1][j], centres[2][k]]
            for a in range(3):
                if (m >> a) & 1:
                    p[a] = p[a] + step
            if vol.intensity is not None:
                c = vol.intensity[k, j, i] + t * (vol.intensity[kn, jn, in_] - vol.intensity[k, j, i])
            else:
                c = np.zeros(fv.shape, F)
        rec["key"].append((i + dx * (j + dy * k.astype(np.int64))) * 8 + m)
        rec["has"].append(has)
        for name, arr in (("x", p[0]), ("y", p[1]), ("z", p[2]), ("nx", n[0]), ("ny", n[1]), ("nz", n[2]), ("c", c)):
            rec[name].append(np.asarray(arr, F))
    if rec["key"]:
        r = {k: np.concatenate(v) for k, v in rec.items()}
    else:
        r = {k: np.zeros(0, bool if k == "has" else np.int64 if k == "key" else F) for k in rec}
    order = np.argsort(r["key"], kind="stable")
    r = {k: v[order] for k, v in r.items()}
    keys = r["key"]

    # rule 4: the known cells with a sign change, in ascending linear index (np.nonzero walks k, then j, then i)
    tri_order, tri_keys = [], []
    if known.any():
        sign = np.zeros((dz, dy, dx), np.int64)
        for e in range(8):
            ez, ey, ex = (e >> 2) & 1, (e >> 1) & 1, e & 1
            sign[:dz - ez, :dy - ey, :dx - ex] |= neg[ez:, ey:, ex:].astype(np.int64) << e
        k, j, i = np.nonzero(known & (sign != 0) & (sign != 255))
        lin = i + dx * (j + dy * k.astype(np.int64))
        s = sign[k, j, i]
        rank = np.arange(lin.size, dtype=np.int64)
        off = [(e & 1) + dx * (((e >> 1) & 1) + dy * (e >> 2)) for e in range(8)]
        for tet, vc in enumerate(TETS):
            case = sum(((s >> vc[n]) & 1) << n for n in range(4))
            for cs in range(1, 15):
                sel = np.nonzero(case == cs)[0]
                if sel.size == 0:
                    continue
                for ti, tri in enumerate(TABLE[cs]):
                    if ODD[tet]:
                        tri = (tri[0], tri[2], tri[1])
                    kk = []
                    for p_, q_ in tri:
                        lo, hi = min(p_, q_), max(p_, q_)  # (the corner of the lower position is a subset of the other)
                        kk.append((lin[sel] + off[vc[lo]]) * 8 + (vc[hi] ^ vc[lo]))
                    tri_keys.append(np.stack(kk, axis=1))
                    tri_order.append(rank[sel] * 12 + tet * 2 + ti)
    if tri_keys:
        tk = np.concatenate(tri_keys)
        tk = tk[np.argsort(np.concatenate(tri_order), kind="stable")]
        idx = np.searchsorted(keys, tk)
        assert idx.max(initial=-1) < keys.size and np.array_equal(keys[idx], tk), "a triangle names a vertex that is not listed"
        triangles = idx.astype(np.int32)
    else:
        triangles = np.zeros((0, 3), np.int32)
    return dict(vertices=np.stack([r["x"], r["y"], r["z"]]).astype(F), normals=np.stack([r["nx"], r["ny"], r["nz"]]).astype(F),
                intensity=r["c"].astype(F), voxel_index=(keys // 8).astype(np.int32), edge=(keys % 8).astype(np.uint8),
                triangles=triangles, n_vertices=int(keys.size), n_triangles=int(triangles.shape[0]),
                n_no_normal=int((~r["has"]).sum()))
