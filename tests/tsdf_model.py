"""numpy restatement of the two rules of the TSDF volume (K19, include/icpk.h): the per-voxel integration rule and the
surface rule.  numpy is used only elementwise, in float32, one rounding per operation in the order the header writes
them (numpy's float32 +, -, *, / and sqrt are correctly rounded and never fused), so that the device and
icpk_tsdf_voxel_update are held against it bit for bit.  The pose is inverted in float64 in the header's order."""
import numpy as np

F = np.float32


def invert_pose(P):
    """[R | t] camera-to-world (4, 4) float64 -> (R^T, -R^T t) as float32, t'_r = -((R_0r t_0 + R_1r t_1) + R_2r t_2)."""
    P = np.asarray(P, np.float64).reshape(4, 4)
    R = P[:3, :3].T.copy()
    t = np.array([-((P[0, r] * P[0, 3] + P[1, r] * P[1, 3]) + P[2, r] * P[2, 3]) for r in range(3)], np.float64)
    return R.astype(F), t.astype(F)


class Volume:
    def __init__(self, dims, voxel, origin, trunc, max_weight=255, depth_scale=5000.0, color=False):
        self.dims = tuple(int(d) for d in dims)
        self.voxel, self.trunc, self.depth_scale = F(voxel), F(trunc), F(depth_scale)
        self.origin = np.asarray(origin, F)
        self.max_weight = int(max_weight)
        dx, dy, dz = self.dims
        self.tsdf = np.zeros((dz, dy, dx), F)
        self.weight = np.zeros((dz, dy, dx), np.uint16)
        self.intensity = np.zeros((dz, dy, dx), F) if color else None

    def centres(self):
        """rule 1 per axis: fl(fl((float)i + 0.5f) * voxel) + origin"""
        return [(np.arange(n).astype(F) + F(0.5)) * self.voxel + self.origin[a] for a, n in enumerate(self.dims)]

    def integrate(self, depth, pose, fx, cx, intensity=None, debug=False):
        """Rules 2 - 11 for one frame; returns n_updated (with debug: also the intermediate arrays)."""
        depth = np.asarray(depth, np.uint16)
        rows, cols = depth.shape
        R, t = invert_pose(pose)
        fx, cx = F(fx), F(cx)
        cxs, cys, czs = self.centres()
        px, py, pz = cxs[None, None, :], cys[None, :, None], czs[:, None, None]
        with np.errstate(all="ignore"):
            q = [((R[r, 0] * px + R[r, 1] * py) + R[r, 2] * pz) + t[r] for r in range(3)]
            front = q[2] > 0
            u = (q[0] * fx) / q[2] + cx
            v = (q[1] * fx) / q[2] + cx
            col = np.floor(u + F(0.5))
            row = np.floor(v + F(0.5))
            inside = front & (col >= 0) & (col < cols) & (row >= 0) & (row < rows)
            ci = np.where(inside, col, 0).astype(np.int64)
            ri = np.where(inside, row, 0).astype(np.int64)
            d = depth[ri, ci]
            seen = inside & (d != 0)
            sdf = d.astype(F) / self.depth_scale - q[2]
            ok = seen & ~(sdf < -self.trunc)
            f = np.minimum(F(1), sdf / self.trunc)
            w = self.weight.astype(F)
            new = ((self.tsdf * w) + f) / (w + F(1))
            self.tsdf = np.where(ok, new, self.tsdf).astype(F)
            if self.intensity is not None:
                c = np.asarray(intensity, F).reshape(rows, cols)[ri, ci]
                newc = ((self.intensity * w) + c) / (w + F(1))
                self.intensity = np.where(ok, newc, self.intensity).astype(F)
        self.weight = np.where(ok, np.minimum(self.weight.astype(np.int64) + 1, self.max_weight), self.weight).astype(np.uint16)
        n = int(ok.sum())
        if debug:
            return n, dict(front=front, inside=inside, seen=seen, ok=ok, u=u, v=v, sdf=sdf, q=q)
        return n

    def _gradient(self, ok, k, j, i):
        """(defined, [g_x, g_y, g_z]) at the voxels (k, j, i): central differences of tsdf, all six neighbours in
        bounds with enough weight"""
        dx, dy, dz = self.dims
        inb = (i >= 1) & (i + 1 < dx) & (j >= 1) & (j + 1 < dy) & (k >= 1) & (k + 1 < dz)
        kc, jc, ic = np.clip(k, 1, max(dz - 2, 1)), np.clip(j, 1, max(dy - 2, 1)), np.clip(i, 1, max(dx - 2, 1))
        if not inb.any():
            return inb, [np.zeros(k.shape, F)] * 3
        f = self.tsdf
        has = inb & ok[kc, jc, ic + 1] & ok[kc, jc, ic - 1] & ok[kc, jc + 1, ic] & ok[kc, jc - 1, ic] & \
            ok[kc + 1, jc, ic] & ok[kc - 1, jc, ic]
        g = [f[kc, jc, ic + 1] - f[kc, jc, ic - 1], f[kc, jc + 1, ic] - f[kc, jc - 1, ic],
             f[kc + 1, jc, ic] - f[kc - 1, jc, ic]]
        return has, g

    def extract(self, min_weight=1):
        """The surface rule.  Returns dict(points (3, n), normals (3, n), intensity, voxel, axis, n_no_normal,
        dropped_voxel, dropped_axis, crossing_points), the list in ascending (voxel, axis); crossing_points: every
        crossing's point, listed or dropped."""
        dx, dy, dz = self.dims
        f = self.tsdf
        ok = self.weight >= min_weight
        centres = self.centres()
        rec = {k: [] for k in ("key", "x", "y", "z", "nx", "ny", "nz", "c", "listed")}
        for axis in range(3):
            sv = [slice(None)] * 3
            sn = [slice(None)] * 3
            sv[2 - axis], sn[2 - axis] = slice(0, -1), slice(1, None)
            sv, sn = tuple(sv), tuple(sn)
            cross = ok[sv] & ok[sn] & ((f[sv] < 0) != (f[sn] < 0))
            k, j, i = np.nonzero(cross)  # (V's own indices: its slice starts at 0)
            step = [(0, 0, 1), (0, 1, 0), (1, 0, 0)][axis]
            kn, jn, in_ = k + step[0], j + step[1], i + step[2]
            fv, fn = f[k, j, i], f[kn, jn, in_]
            with np.errstate(all="ignore"):
                t = fv / (fv - fn)
                hv, gv = self._gradient(ok, k, j, i)
                hn, gn = self._gradient(ok, kn, jn, in_)
                m = [gv[a] + t * (gn[a] - gv[a]) for a in range(3)]
                length = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
                listed = hv & hn & (length > 0)
                n = [m[a] / length for a in range(3)]
                p = [centres[0][i], centres[1][j], centres[2][k]]
                p[axis] = p[axis] + t * self.voxel
                if self.intensity is not None:
                    c = self.intensity[k, j, i] + t * (self.intensity[kn, jn, in_] - self.intensity[k, j, i])
                else:
                    c = np.zeros(fv.shape, F)
            rec["key"].append((i + dx * (j + dy * k.astype(np.int64))) * 3 + axis)
            rec["listed"].append(listed)
            for name, arr in (("x", p[0]), ("y", p[1]), ("z", p[2]), ("nx", n[0]), ("ny", n[1]), ("nz", n[2]), ("c", c)):
                rec[name].append(np.asarray(arr, F))
        r = {k: np.concatenate(v) for k, v in rec.items()}
        order = np.argsort(r["key"], kind="stable")
        r = {k: v[order] for k, v in r.items()}
        keep, drop = r["listed"], ~r["listed"]
        return dict(points=np.stack([r["x"][keep], r["y"][keep], r["z"][keep]]),
                    normals=np.stack([r["nx"][keep], r["ny"][keep], r["nz"][keep]]),
                    intensity=r["c"][keep], voxel=(r["key"][keep] // 3).astype(np.int32),
                    axis=(r["key"][keep] % 3).astype(np.uint8), n_no_normal=int(drop.sum()),
                    dropped_voxel=(r["key"][drop] // 3).astype(np.int64), dropped_axis=(r["key"][drop] % 3).astype(np.uint8),
                    crossing_points=np.stack([r["x"], r["y"], r["z"]]))
