"""The mesh rule of the TSDF volume (K21) without a GPU: icpk_tsdf_mesh_host -- the host half of csrc/tsdf_rule.h, the
header the kernels include -- against tests/tsdf_mesh_model.py bit for bit on every case; the counts the rule was
specified against; what the index list alone proves (orientable, every vertex used, closed where the surface is);
the winding against the vertex normals; the tie to K19's crossings; the accuracy on the analytic room; the PLY round
trip; and the refusals."""
import ctypes as C

import numpy as np
import pytest

import tsdf_cases as tc
import tsdf_mesh_cases as mc
import tsdf_mesh_model as mm
from icp_slam_prototype_amd import binding, build, tsdf


@pytest.fixture(scope="module")
def lib():
    build.build()
    return binding.load()


def host_mesh(name, **kw):
    c = mc.case(name)
    vol = c["volume"]
    return binding.tsdf_mesh_host(mc.params(binding, name), vol.tsdf, vol.weight, vol.intensity, min_weight=c["min_weight"], **kw)


def orientation(m):
    """(triangles whose (b - a) x (c - a) points against n_a + n_b + n_c, triangles without area), in float64 from the
    float32 vertices"""
    v, n, tri = m["vertices"].astype(np.float64), m["normals"].astype(np.float64), m["triangles"]
    if tri.shape[0] == 0:
        return 0, 0
    a, b, c = (v[:, tri[:, k]].T for k in range(3))
    cross = np.cross(b - a, c - a)
    nsum = (n[:, tri[:, 0]] + n[:, tri[:, 1]] + n[:, tri[:, 2]]).T
    return int(((cross * nsum).sum(1) < 0).sum()), int((~cross.any(axis=1)).sum())


@pytest.mark.parametrize("name", mc.ALL)
def test_mesh_host_gives_the_models_bytes(lib, name):
    want, got = mc.model(name), host_mesh(name)
    assert tuple(got[k] for k in mc.COUNTS) == tuple(want[k] for k in mc.COUNTS)
    for k in mc.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k
    if name == "room_color":
        assert got["intensity"].min() >= 0 and got["intensity"].max() <= 1 and np.ptp(got["intensity"]) > 0.1
    else:
        assert not got["intensity"].any()
    if name == "rounds":  # some chunk of 512 voxels owns vertices in both of its rounds of 256
        chunk, half = got["voxel_index"] // 512, (got["voxel_index"] % 512) // 256
        assert np.intersect1d(chunk[half == 0], chunk[half == 1]).size > 100


def test_the_table_is_the_general_rule():
    """the header's table, typed in as the header prints it, against the rule behind it (tsdf_mesh_model.TABLE)"""
    header = {1: "(01,02,03)", 2: "(10,13,12)", 3: "(02,03,13) (02,13,12)", 4: "(20,21,23)", 5: "(01,23,03) (01,21,23)",
              6: "(10,13,23) (10,23,20)", 7: "(30,31,32)", 8: "(30,32,31)", 9: "(01,02,32) (01,32,31)",
              10: "(10,32,12) (10,30,32)", 11: "(20,23,21)", 12: "(20,21,31) (20,31,30)", 13: "(10,12,13)", 14: "(01,03,02)"}
    assert mm.TABLE[0] == [] and mm.TABLE[15] == []
    for case, text in header.items():
        tris = [tuple((int(e[0]), int(e[1])) for e in t.strip("()").split(",")) for t in text.split()]
        assert mm.TABLE[case] == tris, case
    assert mm.TETS == [(0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7)]
    assert mm.ODD == [False, True, True, False, False, True]


@pytest.mark.parametrize("name", tuple(mc.SET))
def test_the_specified_counts_hold(name):
    """`cut`: the float64 restatement the rule was specified with had 16 triangles without area; the float32 rule gives
    28, and that is what is asserted.  Its sphere passes through three lattice points (2.7^2 + 3.6^2 + 2.8^2 = 5.3^2 and
    its like): two come out as exactly 0 in float64 and one as 8.9e-16, and with that one the float32 sum centre +
    fl(t voxel) absorbs the step, so its triangles lose their area as well.  The volume is dyadic, so a triangle
    without area has exactly none and no triangle points inwards (test_no_triangle_points_inwards)."""
    m, top = mc.model(name), mc.topology(mc.model(name))
    inward, flat = orientation(m)
    print(f"{name}: {m['n_vertices']} vertices, {m['n_triangles']} triangles, {m['n_no_normal']} without a normal, {top}, "
          f"{flat} triangles without area, {inward} pointing inwards")
    if name == "flat":
        assert (m["n_vertices"], m["n_triangles"], m["n_no_normal"]) == (0, 0, 0)
        return
    nv, nt, closed, euler, zero_area = mc.SET[name][2]
    assert (m["n_vertices"], m["n_triangles"], top["closed"], top["euler"]) == (nv, nt, closed, euler)
    assert flat == (28 if name == "cut" else zero_area) and inward == 0
    if name == "zeros":
        assert int((mc.case(name)["volume"].tsdf == 0).sum()) == 30
    if name in ("sphere", "torus"):
        assert m["n_no_normal"] == 0


@pytest.mark.parametrize("name", mc.ALL)
def test_what_the_index_list_proves(name):
    m = mc.model(name)
    top = mc.topology(m)
    assert top["orientable"] and top["all_used"]
    tri = m["triangles"]
    assert tri.shape[0] == 0 or (tri.min() >= 0 and tri.max() < m["n_vertices"])
    assert not (tri[:, 0] == tri[:, 1]).any() and not (tri[:, 1] == tri[:, 2]).any() and not (tri[:, 0] == tri[:, 2]).any()
    # the order of the vertex list: ascending (voxel, edge type), no key twice
    key = m["voxel_index"].astype(np.int64) * 8 + m["edge"]
    assert np.all(np.diff(key) > 0) and (m["n_vertices"] == 0 or (m["edge"].min() >= 1 and m["edge"].max() <= 7))
    if name in ("sphere", "torus", "zeros"):
        assert top["closed"] and top["euler"] == {"sphere": 2, "torus": 0, "zeros": 2}[name]
    if name == "cut":
        assert not top["closed"]


@pytest.mark.parametrize("name", mc.ALL)
def test_no_triangle_points_inwards(name):
    m = mc.model(name)
    inward, flat = orientation(m)
    share = m["n_no_normal"] / max(m["n_vertices"], 1)
    print(f"{name}: {m['n_triangles']} triangles, {flat} without area, {inward} pointing inwards; {m['n_no_normal']} of "
          f"{m['n_vertices']} vertices without a normal ({share:.4f})")
    assert inward == 0


@pytest.mark.parametrize("name", mc.ALL)
def test_axis_edge_vertices_are_k19s_crossings(name):
    c, m = mc.case(name), mc.model(name)
    s = c["volume"].extract(c["min_weight"])
    has = m["normals"].any(axis=0)
    sel = np.isin(m["edge"], (1, 2, 4)) & has
    axis = np.log2(m["edge"][sel].astype(np.float64)).astype(np.int64)
    key = m["voxel_index"][sel].astype(np.int64) * 3 + axis
    skey = s["voxel"].astype(np.int64) * 3 + s["axis"]
    at = np.searchsorted(skey, key)
    assert key.size == 0 or (at.max() < skey.size and np.array_equal(skey[at], key))
    assert m["vertices"][:, sel].tobytes() == np.ascontiguousarray(s["points"][:, at]).tobytes()
    assert m["normals"][:, sel].tobytes() == np.ascontiguousarray(s["normals"][:, at]).tobytes()
    assert m["intensity"][sel].tobytes() == np.ascontiguousarray(s["intensity"][at]).tobytes()
    if name in ("sphere", "room", "room_color", "rounds"):
        assert key.size > 500


def test_accuracy_on_the_room():
    """K19 asserts that 99 % of its crossings lie within one voxel edge of the analytic room; the mesh's vertices are held
    to the same bar, the vertices on diagonal edges included.  Measured: see the printed shares."""
    m = mc.model("room")
    dist = tc.room_distance(m["vertices"].astype(np.float64))
    voxel = tc.ROOM_VOLUME["voxel"]
    on_axis = np.isin(m["edge"], (1, 2, 4))
    shares = [float(np.mean(dist[s] < voxel)) for s in (np.ones_like(on_axis), on_axis, ~on_axis)]
    print(f"room: {dist.size} vertices within one voxel of the analytic room: all {shares[0]:.4f}, axis edges {shares[1]:.4f}, "
          f"diagonal edges {shares[2]:.4f}; max {dist.max():.4f} m, median {np.median(dist):.4f} m")
    assert shares[0] >= 0.99 and shares[1] >= 0.99 and shares[2] >= 0.99


def test_ply_round_trip(tmp_path):
    for name in ("room_color", "sphere", "flat"):
        m = dict(mc.model(name), color=name == "room_color")
        path = tmp_path / f"{name}.ply"
        tsdf.write_ply(path, m)
        back = tsdf.read_ply(path)
        assert back["color"] == m["color"]
        for k in ("vertices", "normals", "intensity", "triangles"):
            assert back[k].dtype == m[k].dtype and back[k].shape == m[k].shape and back[k].tobytes() == m[k].tobytes(), (name, k)
        head = path.read_bytes().split(b"end_header\n")[0].decode("ascii").split("\n")
        assert head[:3] == ["ply", "format binary_little_endian 1.0", f"element vertex {m['n_vertices']}"]
        assert ("property float intensity" in head) == m["color"] and f"element face {m['n_triangles']}" in head
        size = len(b"\n".join(h.encode() for h in head)) + len(b"end_header\n")
        assert path.stat().st_size == size + m["n_vertices"] * 4 * (7 if m["color"] else 6) + m["n_triangles"] * 13


def test_mesh_host_refuses_more_than_max_surface(lib):
    """A checkerboard of signs makes every tetrahedron a two-inside case: 12 triangles per cell.  282^3 cells give
    269 109 216 triangles, the smallest cube above ICPK_TSDF_MAX_SURFACE = 2^28 = 268 435 456; the vertices (the axis
    edges and the body diagonal change sign, the face diagonals join voxels of one parity) stay below it.  The refusal comes with the counts, whatever room is offered."""
    d = 283
    i = np.arange(d)
    f = np.where((i[:, None, None] + i[None, :, None] + i[None, None, :]) % 2 == 0, np.float32(0.5), np.float32(-0.5))
    p = binding.tsdf_params(dims=(d, d, d), voxel=0.0625, origin=(0, 0, 0), trunc=0.25)
    w, counts = np.ones(f.shape, np.uint16), np.full(3, -1, np.int64)
    rc = lib.icpk_tsdf_mesh_host(C.byref(p), 1, f.ctypes.data_as(C.POINTER(C.c_float)), w.ctypes.data_as(C.POINTER(C.c_uint16)),
                                 None, 1 << 40, 1 << 40, *([None] * 10), counts.ctypes.data_as(C.POINTER(C.c_int64)))
    nv = 3 * d * d * (d - 1) + (d - 1) ** 3  # (the three axis edges and the body diagonal whose far end is in range)
    assert rc == binding.E_ARG and tuple(counts[:2]) == (nv, 12 * (d - 1) ** 3)
    assert nv < binding.TSDF_MAX_SURFACE < 12 * (d - 1) ** 3


def test_refusals_of_mesh_host(lib):
    want = mc.model("sphere")
    nv, nt = want["n_vertices"], want["n_triangles"]
    # the capacity refusal fills counts; a capacity that is just enough is fine
    for caps in (dict(cap_vertices=nv - 1, cap_triangles=nt), dict(cap_vertices=nv, cap_triangles=nt - 1),
                 dict(cap_vertices=0, cap_triangles=0)):
        with pytest.raises(binding.IcpkError) as e:
            host_mesh("sphere", **caps)
        assert e.value.code == binding.E_ARG and e.value.counts == (nv, nt, 0)
    got = host_mesh("sphere", cap_vertices=nv, cap_triangles=nt)
    assert got["triangles"].tobytes() == want["triangles"].tobytes()
    roomy = host_mesh("sphere", cap_vertices=nv + 7, cap_triangles=nt + 5)
    assert roomy["vertices"].tobytes() == want["vertices"].tobytes() and roomy["n_triangles"] == nt
    assert host_mesh("flat")["n_vertices"] == 0 and host_mesh("flat", cap_vertices=0, cap_triangles=0)["triangles"].shape == (0, 3)

    vol = mc.case("sphere")["volume"]
    p = mc.params(binding, "sphere")
    f, w = np.ascontiguousarray(vol.tsdf).reshape(-1), np.ascontiguousarray(vol.weight).reshape(-1)
    counts = np.zeros(3, np.int64)
    fp, u16 = C.POINTER(C.c_float), C.POINTER(C.c_uint16)

    def call(params=p, min_weight=1, tsdf=f, weight=w, intensity=None, cv=0, ct=0, cnt=counts):
        return lib.icpk_tsdf_mesh_host(None if params is None else C.byref(params), min_weight,
                                       None if tsdf is None else tsdf.ctypes.data_as(fp),
                                       None if weight is None else weight.ctypes.data_as(u16),
                                       None if intensity is None else intensity.ctypes.data_as(fp), cv, ct, *([None] * 10),
                                       None if cnt is None else cnt.ctypes.data_as(C.POINTER(C.c_int64)))

    assert call(cv=nv, ct=nt) == 0 and tuple(counts) == (nv, nt, 0)  # (every array NULL: the counts alone)
    for kw in (dict(params=None), dict(tsdf=None), dict(weight=None), dict(cnt=None), dict(min_weight=0), dict(min_weight=65536),
               dict(cv=-1), dict(ct=-1), dict(intensity=np.zeros(f.size, np.float32)),
               dict(params=binding.tsdf_params(dims=(0, 4, 4), voxel=0.1, origin=(0, 0, 0), trunc=0.2))):
        assert call(**kw) == binding.E_ARG, kw
    pc = mc.params(binding, "room_color")
    big, bw = np.zeros(64 ** 3, np.float32), np.zeros(64 ** 3, np.uint16)
    assert call(params=pc, tsdf=big, weight=bw) == binding.E_ARG  # (a colour volume wants its intensity plane)
    assert call(params=pc, tsdf=big, weight=bw, intensity=big) == 0 and tuple(counts) == (0, 0, 0)
    assert call(min_weight=2, cv=nv, ct=nt) == 0 and tuple(counts) == (0, 0, 0)  # (weight 1 everywhere: nothing is known)
