"""icp::TsdfVolume::deintegrate / apply / refuse (tests/cpp/test_tsdf_refuse.cpp) on ten frames of the room -- two
batches of refuse -- against the same calls made through the Python binding, byte for byte."""
import struct

import numpy as np
import pytest

import mirror
import tsdf_apply_cases as ac
import tsdf_cases as tc
from icp_slam_prototype_amd import binding
from icp_slam_prototype_amd.tsdf import TsdfVolume

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("color", [False, True])
def test_cpp_refuse_equals_binding(color):
    v = tc.ROOM_VOLUME
    motions = [((0.0, 2.0 * k - 9.0, 0.0), (0.03 * k - 0.1, 0.0, 0.01 * k)) for k in range(10)]
    depths = [tc.room_frame(*m)[0] for m in motions]
    new = [tc.pose(*m) for m in motions]
    old = [ac.drift(P, (0.2 * k, -0.3 * k, 0.1 * k), (0.005 * k, -0.002 * k, 0.0)) for k, P in enumerate(new)]
    inten = [tc.room_intensity(*m) for m in motions] if color else None
    rows, cols = depths[0].shape
    parts = [struct.pack("<8i", *v["dims"], 255, binding.TSDF_COLOR if color else 0, rows, cols, len(depths)),
             np.float32([v["voxel"], *v["origin"], v["trunc"], tc.ROOM_FX, tc.ROOM_CX, 0]).tobytes()]
    for k, d in enumerate(depths):
        parts.append(np.ascontiguousarray(old[k], np.float64).tobytes() + np.ascontiguousarray(new[k], np.float64).tobytes())
        parts.append(np.ascontiguousarray(d, np.uint16).tobytes())
        if color:
            parts.append(np.ascontiguousarray(inten[k], np.float32).tobytes())
    raw, stdout = mirror.run("test_tsdf_refuse", b"".join(parts))
    with binding.Context(0) as ctx:
        vol = TsdfVolume(ctx, color=color, fx=tc.ROOM_FX, cx=tc.ROOM_CX, **v)
        vol.integrate_all(depths, old, inten)
        taken = vol.deintegrate(depths[-1], old[-1], None if inten is None else inten[-1])
        put = vol.apply([depths[-1]], [(+1, 0, old[-1])], None if inten is None else [inten[-1]])
        moved = vol.refuse(depths, old, new, inten)
        planes = vol.planes(intensity=color)
    want = moved.astype(np.int64).tobytes() + struct.pack("<i", taken) + put.astype(np.int64).tobytes()
    want += b"".join(a.tobytes() for a in planes if a is not None)
    assert taken == put[0] > 1000 and moved.min() > 1000 and planes[1].max() == 10 and raw == want
    assert f"refused 10 frames; the last one: {taken} voxels out, {put[0]} back in" in stdout
