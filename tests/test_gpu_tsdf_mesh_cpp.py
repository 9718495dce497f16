"""icp::TsdfVolume::extractMesh / getMesh / setPlanes (tests/cpp/test_tsdf_mesh.cpp) on the room case, with and without
colour, against the same calls made through the Python binding, byte for byte: the counts, the vertices with their keys
and the triangles.  The program itself checks that the planes read back and handed to setPlanes give the same mesh."""
import struct

import numpy as np
import pytest

import mirror
import tsdf_cases as tc
from icp_slam_prototype_amd import binding

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["room", "room_color"])
def test_cpp_mesh_equals_binding(name):
    c = tc.case(name)
    v = c["volume"]
    color = bool(v.get("color"))
    rows, cols = c["frames"][0][0].shape
    parts = [struct.pack("<8i", *v["dims"], 255, binding.TSDF_COLOR if color else 0, rows, cols, len(c["frames"])),
             np.float32([v["voxel"], *v["origin"], v["trunc"], c["fx"], c["cx"], 0]).tobytes()]
    for d, Pf, img in c["frames"]:
        parts.append(np.ascontiguousarray(Pf, np.float64).tobytes())
        parts.append(np.ascontiguousarray(d, np.uint16).tobytes())
        if color:
            parts.append(np.ascontiguousarray(img, np.float32).tobytes())
    parts.append(struct.pack("<i", 1))
    raw, stdout = mirror.run("test_tsdf_mesh", b"".join(parts))
    with binding.Context(0) as ctx:
        ctx.tsdf_create(dims=v["dims"], voxel=v["voxel"], origin=v["origin"], trunc=v["trunc"],
                        flags=binding.TSDF_COLOR if color else 0)
        for d, Pf, img in c["frames"]:
            ctx.tsdf_integrate(d, Pf, img, fx=c["fx"], cx=c["cx"])
        nv, nt, nn = ctx.tsdf_extract_mesh(1)
        m = ctx.tsdf_get_mesh()
    assert struct.unpack_from("<4i", raw, 0) == (nv, nt, nn, 0) and nv > 10000 and nt > 20000
    want = b"".join(np.ascontiguousarray(a).tobytes() for a in (*m["vertices"], *m["normals"], m["intensity"], m["voxel_index"],
                                                                 m["edge"], m["triangles"]))
    assert len(want) == 33 * nv + 12 * nt and raw[16:] == want
    assert bool(m["intensity"].any()) == color
    assert f"mesh: {nv} vertices, {nt} triangles, {nn} without a normal" in stdout
