"""Sequential restatement of the reference's certainty map (map.hpp, map.cpp) in plain Python: the voxel mapping of
getVoxelCoordinates (map.cpp:55-85), the three update rules (map.cpp:88-119, :122-206, :220-269), the lookup table
(one slot per voxel, shared by both lists) and the two point lists.  Points are applied one by one in input order,
exactly as the reference's loops do.  Test infrastructure: the device map is checked against it.

Slots hold (list, index) of the point that filled them instead of the point itself (the library drops colour, so the
reference's comparison with an empty color_point_t becomes "filled yet"); both give the same behaviour except for a
point at exactly (0, 0, 0), which the library documents as unpinned.
"""
import numpy as np

MAP_HEIGHT = 300  # map.hpp:9
MAX_CONFIDENCE = 180  # map.hpp:13
DELTA_CONFIDENCE = 25  # map.hpp:11
C = np.float32(10.0) / np.float32(MAP_HEIGHT)  # map.hpp:17 / map.cpp:58: float(10.0f / 300.0f)
KEYPOINTS, POINTS = 0, 1
ADD_CLOUD, ADD_ASSOCIATED, ADD_UNASSOCIATED = 0, 1, 2
INT_MIN = -(2 ** 31)


def cvttss2si(q):
    """int(float) as the reference's x86 build converts it: truncation toward zero, INT_MIN for NaN, +-inf and
    |q| >= 2^31."""
    q = np.float32(q)
    if not np.isfinite(q) or q >= np.float32(2.0 ** 31) or q < np.float32(-(2.0 ** 31)):
        return INT_MIN
    return int(q)  # Python int() truncates toward zero


def voxel(p):
    """map.cpp:55-85: per axis int(p / c) (float division), clamped to [0, 299]."""
    out = []
    with np.errstate(all="ignore"):
        for v in p:
            i = cvttss2si(np.float32(v) / C)
            out.append(min(max(i, 0), MAP_HEIGHT - 1))
    return tuple(out)


class Map:
    """map::Map with the grid as a dict (voxel -> certainty, absent = 0) and the lookup table as a dict
    (voxel -> (list, index))."""

    def __init__(self):  # map.cpp:17-31
        self.reset()

    def reset(self):
        self.cert = {}
        self.slot = {}
        self.lists = ([], [])  # key points, points: (x, y, z) float32 triples

    def certainty(self, v):
        return self.cert.get(v, 0)

    def _fill(self, v, p, lst):
        if v not in self.slot:
            self.slot[v] = (lst, len(self.lists[lst]))
            self.lists[lst].append(tuple(np.float32(c) for c in p))

    def add(self, rule, p, d):
        """one point through one rule"""
        assert 1 <= d <= 255
        v = voxel(p)
        c = self.certainty(v)
        if rule == ADD_CLOUD:  # map.cpp:249-259
            c = 255 if c > 255 - d else c + d
            self.cert[v] = c
            if c >= MAX_CONFIDENCE:
                self._fill(v, p, KEYPOINTS)
        elif rule == ADD_ASSOCIATED:  # map.cpp:104-113
            if c > 255 - d:
                self.cert[v] = 255
                self._fill(v, p, POINTS)
            else:
                self.cert[v] = c + d
        elif rule == ADD_UNASSOCIATED:  # map.cpp:139-149
            if c >= MAX_CONFIDENCE - d:
                self.cert[v] = 255
                self._fill(v, p, KEYPOINTS)
            else:
                self.cert[v] = c + d
        else:
            raise ValueError(rule)

    def update(self, rule, pts, d, indices=None):
        """pts: (3, n); indices: order of application (None: 0 .. n-1)"""
        pts = np.asarray(pts, np.float32)
        order = range(pts.shape[1]) if indices is None else indices
        for i in order:
            self.add(rule, pts[:, i], d)

    def set_points(self, pts):  # icp.cpp:63: the point list replaced, grid and slots untouched
        pts = np.asarray(pts, np.float32)
        self.lists = (self.lists[0], [tuple(pts[:, i]) for i in range(pts.shape[1])])

    def is_occupied(self, p):  # map.cpp:441-444
        return self.certainty(voxel(p)) >= MAX_CONFIDENCE

    def list_array(self, lst):
        a = np.array(self.lists[lst], np.float32).reshape(-1, 3)
        return np.ascontiguousarray(a.T)

    def grid(self):
        """the dense (300, 300, 300) uint8 grid, [x, y, z]"""
        g = np.zeros((MAP_HEIGHT,) * 3, np.uint8)
        for v, c in self.cert.items():
            g[v] = c
        return g

    def query_slot(self, p):
        return self.slot.get(voxel(p), (-1, -1))
