"""The signed updates of the TSDF volume (K30) as a thread script, in the style of tests/frame_view_thread_cases.py: one
function that makes every call of the family on a context it is handed and returns its outputs as a list of (label,
bytes).  tests/test_gpu_tsdf_apply_threads.py runs it alone on fresh contexts, then on eight threads at once, each thread
on contexts of its own, and compares byte for byte.

The calls: icpk_tsdf_apply on the coloured room (16 ops over two frames), on the 513-voxel tail volume and on the tiny
one -- three shapes of volume and two of n_frames on one context --, icpk_tsdf_deintegrate after an integration, and
TsdfVolume.refuse over ten frames (two batches)."""
import numpy as np

import tsdf_apply_cases as ac
import tsdf_cases as tc
from icp_slam_prototype_amd import binding
from icp_slam_prototype_amd.tsdf import TsdfVolume

from pyramid_thread_cases import first_difference  # noqa: F401 (the comparison the thread test uses)

APPLY_CASES = ("room_color", "tail", "tiny")


def _planes(ctx, color):
    return b"".join(a.tobytes() for a in ctx.tsdf_get(intensity=color) if a is not None)


def script(ctx):
    """Every call of the family, on `ctx`.  Returns [(label, bytes)]."""
    out = []
    for name in APPLY_CASES:
        c = ac.case(name)
        v = c["volume"]
        color = bool(v.get("color"))
        ctx.tsdf_create(dims=v["dims"], voxel=v["voxel"], origin=v["origin"], trunc=v["trunc"],
                        flags=binding.TSDF_COLOR if color else 0)
        n = binding.tsdf_apply(ctx, c["frames"], c["ops"], c["intensities"], fx=c["fx"], cx=c["cx"])
        out.append((f"{name}.counts", n.astype(np.int64).tobytes()))
        out.append((f"{name}.planes", _planes(ctx, color)))
    r = tc.case("room_color")
    vol = TsdfVolume(ctx, color=True, fx=r["fx"], cx=r["cx"], **tc.ROOM_VOLUME)
    for d, P, img in r["frames"]:
        vol.integrate(d, P, img)
    d, P, img = r["frames"][1]
    out.append(("deintegrate", np.int64(vol.deintegrate(d, P, img)).tobytes() + _planes(ctx, True)))
    depths = [f[0] for f in r["frames"]] * 3 + [r["frames"][0][0]]
    inten = [f[2] for f in r["frames"]] * 3 + [r["frames"][0][2]]
    new = [f[1] for f in r["frames"]] * 3 + [r["frames"][0][1]]
    old = [ac.drift(P, (0.2 * k, -0.3 * k, 0.0), (0.004 * k, 0.0, -0.002 * k)) for k, P in enumerate(new)]
    vol = TsdfVolume(ctx, color=True, fx=r["fx"], cx=r["cx"], **tc.ROOM_VOLUME)
    vol.integrate_all(depths, old, inten)
    moved = vol.refuse(depths, old, new, inten)
    out.append(("refuse", moved.astype(np.int64).tobytes() + _planes(ctx, True)))
    return out


def model_outputs():
    """{label: bytes} of the outputs the model states"""
    want = {}
    for name in APPLY_CASES:
        m = ac.model(name)
        want[f"{name}.counts"] = np.int64(m["counts"]).tobytes()
        want[f"{name}.planes"] = b"".join(a.tobytes() for a in (m["tsdf"], m["weight"], m["intensity"]) if a is not None)
    return want
