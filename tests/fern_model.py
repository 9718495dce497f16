"""THE FERN RULE of include/icpk.h (K27) restated in numpy and Python integers: table, encode, dissimilarity, search,
harvest.  Shared by tests/test_fern_host.py, tests/test_gpu_fern.py, tests/test_gpu_fern_threads.py,
tests/test_gpu_fern_cpp.py and tests/test_gpu_relocalise.py, with the scene they run."""
import functools

import numpy as np

import pyramid_model as pm
import tsdf_cases as tc
from icp_slam_prototype_amd import synth

M64 = (1 << 64) - 1
MAX_K = 8
DEFAULTS = dict(level=2, n_ferns=256, seed=27, d_min=1000, d_max=20000, capacity=4096, harvest_above=51, min_valid=128)


def params(**kw):
    """the defaults with fields replaced; harvest_above and min_valid follow n_ferns unless given"""
    p = dict(DEFAULTS, **kw)
    if "n_ferns" in kw:
        p["harvest_above"] = kw.get("harvest_above", p["n_ferns"] // 5)
        p["min_valid"] = kw.get("min_valid", p["n_ferns"] // 2)
    return p


def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, f, j):
    return mix((seed + (f + 1) * 0x9E3779B97F4A7C15 + j * 0xD1B54A32D192ED03) & M64) >> 32


def table(p, rows, cols):
    """(F, 6) int32: row, col, tau_0 .. tau_3"""
    out = np.zeros((p["n_ferns"], 6), np.int32)
    for f in range(p["n_ferns"]):
        out[f, 0] = draw(p["seed"], f, 0) % rows
        out[f, 1] = draw(p["seed"], f, 1) % cols
        for k in range(4):
            out[f, 2 + k] = p["d_min"] + draw(p["seed"], f, 2 + k) % (p["d_max"] - p["d_min"])
    return out


def encode(p, level, tab=None):
    """(code (F / 8,) uint32, V) of a (rows, cols) uint16 level"""
    level = np.asarray(level, np.uint16)
    tab = table(p, *level.shape) if tab is None else tab
    d = level[tab[:, 0], tab[:, 1]].astype(np.int64)
    nib = np.zeros(len(tab), np.uint32)
    for k in range(4):
        nib |= (d > tab[:, 2 + k]).astype(np.uint32) << np.uint32(k)
    nib = nib.reshape(-1, 8)
    code = np.zeros(nib.shape[0], np.uint32)
    for j in range(8):
        code |= nib[:, j] << np.uint32(4 * j)
    return code, int((d != 0).sum())


def nibbles(code):
    code = np.asarray(code, np.uint32)
    return (code[..., None] >> (4 * np.arange(8, dtype=np.uint32))) & np.uint32(15)


def diss(a, b):
    """the ferns whose nibbles differ; broadcasts over leading axes"""
    return (nibbles(a) != nibbles(b)).sum(axis=(-1, -2))


def search(codes, query, k):
    """the min(k, n) keyframes in ascending (diss, index) order: (index, diss) int32 arrays"""
    codes = np.asarray(codes, np.uint32).reshape(-1, np.asarray(query).size)
    if len(codes) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    d = diss(codes, np.asarray(query, np.uint32)[None])
    order = np.lexsort((np.arange(len(d)), d))[:k]
    return order.astype(np.int32), d[order].astype(np.int32)


def harvest(p, V, codes, code):
    n = len(codes)
    if V < p["min_valid"] or n >= p["capacity"]:
        return False
    return n == 0 or int(search(codes, code, 1)[1][0]) > p["harvest_above"]


class Database:
    """the per-frame call on the host: process(level, pose or None, k) -> dict(index, diss, valid, added)"""

    def __init__(self, p, rows, cols):
        self.p, self.tab = p, table(p, rows, cols)
        self.codes, self.poses = [], []

    def process(self, level, pose=None, k=3):
        code, V = encode(self.p, level, self.tab)
        index, d = search(self.codes, code, k)
        added = -1
        if pose is not None and harvest(self.p, V, self.codes, code):
            added = len(self.codes)
            self.codes.append(code)
            self.poses.append(np.array(pose, np.float64).reshape(4, 4))
        return dict(index=index, diss=d, valid=V, added=added, code=code)


# ---- the scene ------------------------------------------------------------------------------------------------------
SCENE_FRAMES, SCENE_K, SCENE_LEVEL = 33, 91, 2
SCENE_KEYFRAMES = [0, 3, 11, 18, 23, 29]
SCENE_MAX_GAP, NOISE = 4, 0.002


def scene_pose(i, extreme=24.0, n=SCENE_FRAMES):
    """frame i on the arc from -extreme degrees about y in steps of 1.5 degrees and 15 mm of x (n = 2 extreme / 1.5 + 1
    frames reach +extreme)"""
    assert n == int(round(2 * extreme / 1.5)) + 1
    return tc.pose((0.0, -extreme + 1.5 * i, 0.0), (-extreme / 100.0 + 0.015 * i, 0.0, 0.0))


def render(P, rng):
    return synth.render_room_depth(tc.ROOM_SHAPE[0], tc.ROOM_SHAPE[1], P[:3, :3], P[:3, 3], tc.ROOM_FX, tc.ROOM_CX, NOISE, rng)


@functools.lru_cache(maxsize=None)
def scene(extreme=24.0, n=SCENE_FRAMES):
    """dict(frames, poses, queries): the trajectory rendered from one default_rng(27) in order, and every frame rendered
    again from default_rng(1000 + i).  Read-only."""
    rng = np.random.default_rng(27)
    poses = [scene_pose(i, extreme, n) for i in range(n)]
    frames = [render(P, rng) for P in poses]
    queries = [render(P, np.random.default_rng(1000 + i)) for i, P in enumerate(poses)]
    for a in frames + queries + poses:
        a.setflags(write=False)
    return dict(frames=frames, poses=poses, queries=queries)


@functools.lru_cache(maxsize=None)
def scene_levels(which="frames", extreme=24.0, n=SCENE_FRAMES, level=SCENE_LEVEL):
    out = [pm.pyramid(d, level + 1, SCENE_K)[level] for d in scene(extreme, n)[which]]
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def scene_harvest(extreme=24.0, n=SCENE_FRAMES, count=None):
    """the model's database after the first `count` frames (default: all), and the per-frame results"""
    s = scene(extreme, n)
    levels = scene_levels("frames", extreme, n)
    db = Database(params(), *levels[0].shape)
    results = [db.process(levels[i], s["poses"][i]) for i in range(n if count is None else count)]
    return db, results
