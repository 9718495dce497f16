"""icp::TsdfVolume (tests/cpp/test_tsdf.cpp) on the room case against the same calls made through the Python binding,
byte for byte: the planes, the counts and the surface list."""
import struct

import numpy as np
import pytest

import mirror
import tsdf_cases as tc
from icp_slam_prototype_amd import binding

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["room", "room_color"])
def test_cpp_tsdf_volume_equals_binding(name):
    c = tc.case(name)
    v = c["volume"]
    color = bool(v.get("color"))
    rows, cols = c["frames"][0][0].shape
    n = int(np.prod(v["dims"]))
    parts = [struct.pack("<8i", *v["dims"], 255, binding.TSDF_COLOR if color else 0, rows, cols, len(c["frames"])),
             np.float32([v["voxel"], *v["origin"], v["trunc"], c["fx"], c["cx"], 0]).tobytes()]
    for d, P, img in c["frames"]:
        parts.append(np.ascontiguousarray(P, np.float64).tobytes())
        parts.append(np.ascontiguousarray(d, np.uint16).tobytes())
        if color:
            parts.append(np.ascontiguousarray(img, np.float32).tobytes())
    raw, stdout = mirror.run("test_tsdf", b"".join(parts))
    with binding.Context(0) as ctx:
        ctx.tsdf_create(dims=v["dims"], voxel=v["voxel"], origin=v["origin"], trunc=v["trunc"],
                        flags=binding.TSDF_COLOR if color else 0)
        updated = [ctx.tsdf_integrate(d, P, img, fx=c["fx"], cx=c["cx"]) for d, P, img in c["frames"]]
        npts, ndrop = ctx.tsdf_extract_surface(1)
        f, w, ci = ctx.tsdf_get(intensity=color)
        s = ctx.tsdf_get_surface()
    k = len(updated)
    assert list(struct.unpack_from(f"<{k}i", raw, 0)) == updated
    assert struct.unpack_from("<2i", raw, 4 * k) == (npts, ndrop) and npts > 1000
    want = f.tobytes() + w.tobytes() + (ci.tobytes() if color else b"")
    want += b"".join(np.ascontiguousarray(a).tobytes() for a in (s["points"][0], s["points"][1], s["points"][2], s["normals"][0],
                                                                s["normals"][1], s["normals"][2], s["intensity"]))
    want += s["voxel"].tobytes() + s["axis"].tobytes()
    assert len(raw) == 4 * k + 8 + len(want) and len(want) == n * (10 if color else 6) + 33 * npts
    assert raw[4 * k + 8:] == want
    assert stdout.count("frame ") == k and f"surface: {npts} points, {ndrop} without a normal" in stdout
