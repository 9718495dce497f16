"""The mesh cases (K21) shared by tests/test_tsdf_mesh_host.py and tests/test_gpu_tsdf_mesh.py.  SET cases hand the
volume an analytic field (computed in float64 in voxel-index units, stored as float32(clip(d / 3, -1, 1)), weight 1
everywhere); FUSED cases are volumes of tsdf_cases with a min_weight; `rounds` is one room frame in a volume whose
chunks take two rounds of 256 voxels.  Every volume and every model mesh is computed once per process and handed out
read-only."""
import functools

import numpy as np

import tsdf_cases as tc
import tsdf_mesh_model as mm
import tsdf_model

SET_VOLUME = dict(voxel=0.0625, origin=(-0.5, -0.375, 0.25), trunc=0.1875)


def _grid(dims):
    dx, dy, dz = dims
    k, j, i = np.meshgrid(np.arange(dz, dtype=np.float64), np.arange(dy, dtype=np.float64), np.arange(dx, dtype=np.float64),
                          indexing="ij")
    return i, j, k


def _sphere(dims, centre, radius):
    i, j, k = _grid(dims)
    return np.sqrt((i - centre[0]) ** 2 + (j - centre[1]) ** 2 + (k - centre[2]) ** 2) - radius


def _torus(dims, centre, major, minor):
    i, j, k = _grid(dims)
    ring = np.sqrt((i - centre[0]) ** 2 + (j - centre[1]) ** 2) - major
    return np.sqrt(ring ** 2 + (k - centre[2]) ** 2) - minor


# name -> (dims, the field, (vertices, triangles, closed, Euler characteristic, zero-area triangles) or None)
SET = {
    "sphere": ((16, 16, 16), lambda d: _sphere(d, (7.3, 7.6, 7.45), 5.3), (1554, 3104, True, 2, 0)),
    "torus": ((24, 24, 12), lambda d: _torus(d, (11.4, 11.7, 5.45), 7.2, 2.6), (3388, 6776, True, 0, 0)),
    "zeros": ((16, 16, 16), lambda d: _sphere(d, (8.0, 8.0, 8.0), 5.0), (1298, 2592, True, 2, 228)),
    "cut": ((16, 16, 16), lambda d: _sphere(d, (7.3, 7.6, 2.2), 5.3), (1134, 2198, False, 1, 16)),
    "flat": ((16, 16, 1), lambda d: _sphere(d, (7.3, 7.6, 0.2), 5.3), None),
}
# name -> (case of tsdf_cases, min_weight)
FUSED = {"room": ("room", 1), "room_color": ("room_color", 1), "odd": ("odd", 1), "holes": ("holes", 1), "plane": ("plane", 1),
         "room_min_weight_2": ("room", 2)}
# 160 x 144 x 96 = 2 211 840 voxels: ceil(n / 8192) = 270, so a chunk is 512 voxels and takes two rounds
ROUNDS_VOLUME = dict(dims=(160, 144, 96), voxel=0.032, origin=(-2.56, -2.56, 0.9), trunc=0.128)
ALL = tuple(SET) + tuple(FUSED) + ("rounds",)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(volume: the tsdf_model.Volume with its planes, min_weight, set: whether the planes are handed over by
    icpk_tsdf_set, frames / fx / cx: what is integrated otherwise, params: keywords of binding.tsdf_params)"""
    if name in SET:
        dims, field, _ = SET[name]
        vol = tsdf_model.Volume(dims=dims, **SET_VOLUME)
        vol.tsdf = np.clip(field(dims) / 3.0, -1.0, 1.0).astype(np.float32)
        vol.weight = np.ones(vol.tsdf.shape, np.uint16)
        out = dict(volume=vol, min_weight=1, set=True, params=dict(dims=dims, **SET_VOLUME))
    elif name == "rounds":
        d, P = tc.room_frame(*tc.ROOM_MOTIONS[0])
        vol = tsdf_model.Volume(**ROUNDS_VOLUME)
        vol.integrate(d, P, tc.ROOM_FX, tc.ROOM_CX)
        out = dict(volume=vol, min_weight=1, set=False, frames=[(d, P, None)], fx=tc.ROOM_FX, cx=tc.ROOM_CX,
                   params=dict(ROUNDS_VOLUME))
    else:
        src, min_weight = FUSED[name]
        c = tc.case(src)
        v = c["volume"]
        out = dict(volume=tc.model(src)["volume"], min_weight=min_weight, set=False, frames=c["frames"], fx=c["fx"], cx=c["cx"],
                   params=dict(dims=v["dims"], voxel=v["voxel"], origin=v["origin"], trunc=v["trunc"],
                               max_weight=v.get("max_weight"), color=bool(v.get("color"))))
    for a in (out["volume"].tsdf, out["volume"].weight):
        a.flags.writeable = False
    return out


def params(binding, name):
    p = dict(case(name)["params"])
    color = p.pop("color", False)
    return binding.tsdf_params(flags=binding.TSDF_COLOR if color else 0, **p)


@functools.lru_cache(maxsize=None)
def model(name):
    """tsdf_mesh_model.mesh over the case; arrays are read-only"""
    c = case(name)
    out = mm.mesh(c["volume"], c["min_weight"])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return out


ARRAYS = ("vertices", "normals", "intensity", "voxel_index", "edge", "triangles")
COUNTS = ("n_vertices", "n_triangles", "n_no_normal")


def directed_edges(tri):
    """the 3 m directed edges of the (m, 3) index list as one int64 each"""
    t = np.asarray(tri, np.int64)
    a = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    b = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    return a << 32 | b, b << 32 | a


def topology(m):
    """dict(orientable: no directed edge twice, all_used: every vertex in a triangle, closed: every directed edge has its
    reverse, euler: V - E + F over undirected edges)"""
    tri, n = m["triangles"], m["n_vertices"]
    if tri.shape[0] == 0:
        return dict(orientable=True, all_used=n == 0, closed=True, euler=0)
    fwd, rev = directed_edges(tri)
    t = np.asarray(tri, np.int64)
    lo, hi = np.minimum(t, np.roll(t, -1, axis=1)), np.maximum(t, np.roll(t, -1, axis=1))
    undirected = np.unique(lo.ravel() << 32 | hi.ravel()).size
    return dict(orientable=np.unique(fwd).size == fwd.size, all_used=np.unique(tri).size == n,
                closed=bool(np.isin(rev, fwd).all()), euler=n - undirected + tri.shape[0])
