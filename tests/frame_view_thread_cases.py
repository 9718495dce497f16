"""The frame view family (K28) as a thread script, in the style of tests/projective_thread_cases.py: one function that
makes every call of the family on a context it is handed and returns its outputs as a list of (label, bytes).  tests/
test_gpu_frame_view_threads.py runs it alone on fresh contexts, then on eight threads at once, each thread on contexts
of its own, and compares byte for byte.

The calls: the build of the coloured room view (three levels in one launch) with its counts and planes; the gradients
of two levels; through ICPK_VIEW_FRAME on levels 0 and 1 the 10-iteration loop with its trace, one reduction and the
per-pixel association against the room's fourth frame, geometric and coloured; a small build; and two frames of
odometry.ProjectiveOdometry."""
import numpy as np

import frame_view_cases as fc
import tsdf_cases as tc
from icp_slam_prototype_amd import binding, depth
from icp_slam_prototype_amd.odometry import ProjectiveOdometry

from pyramid_thread_cases import first_difference  # noqa: F401 (the comparison the thread test uses)


def script(ctx):
    """Every call of the family, on `ctx`.  Returns [(label, bytes)]."""
    out = []
    k, f = fc.case("room_color"), fc.next_frame()
    fc.device_setup(ctx, "room_color", depth)
    counts = binding.frame_view_build(ctx, k["pose"], fx=k["fx"], cx=k["cx"])
    out.append(("room_color.counts", np.int32(counts).tobytes()))
    for l in range(3):
        out.append((f"room_color.planes{l}", binding.frame_view(ctx, l).tobytes()))
    for l in (0, 1):
        binding.frame_view_color_gradients(ctx, l, fc.GRADIENT_RADIUS * 2 ** l)
        out.append((f"room_color.gradients{l}", binding.frame_view_get_color_gradients(ctx, l).tobytes()))
    depth.build_pyramid(ctx, f["depth"], depth.pyramid_params(levels=3), intensity=f["intensity"])
    for l in (0, 1):
        binding.projective_set_view(ctx, binding.VIEW_FRAME, l)
        p = binding.default_projective_params(level=l, fx=k["fx"], cx=k["cx"])
        for tag, align in (("geo", binding.align_projective), ("col", binding.align_projective_colored)):
            pose, res = align(ctx, k["pose"], p)
            out.append((f"l{l}.{tag}.pose", pose.tobytes() + bytes(res)))
            for i, t in enumerate(binding.projective_trace(ctx)):
                out.append((f"l{l}.{tag}.trace{i}", t["pose"].tobytes() + t["sums"].tobytes() + np.int64([t["count"], t["status"]]).tobytes()))
        sums, count = binding.projective_reduce(ctx, k["pose"], p)
        out.append((f"l{l}.sums", sums.tobytes() + np.int64(count).tobytes()))
        pixel, dist = binding.projective_associate(ctx, k["pose"], p)
        out.append((f"l{l}.pairs", pixel.tobytes() + dist.tobytes()))
    binding.projective_set_view(ctx, binding.VIEW_RAYCAST)
    fc.device_setup(ctx, "5x7_hole", depth)
    h = fc.case("5x7_hole")
    counts = binding.frame_view_build(ctx, h["pose"], fx=h["fx"], cx=h["cx"])
    out.append(("5x7_hole.view", np.int32(counts).tobytes() + binding.frame_view(ctx, 0).tobytes()))
    odo = ProjectiveOdometry(ctx, pose=k["pose"], fx=k["fx"], cx=k["cx"])
    odo.track(k["depth"])
    out.append(("odometry.pose", odo.track(f["depth"]).tobytes() + b"".join(bytes(st) for st in odo.level_stats)))
    binding.frame_view_release(ctx)
    return out


def model_outputs():
    """{label: bytes} of the outputs the models state"""
    import gicp_model
    import projective_model as jm
    want = {}
    e = [fc.expected("room_color", l) for l in range(3)]
    want["room_color.counts"] = np.int32([[x["n_valid"] for x in e], [x["n_no_normal"] for x in e]]).tobytes()
    for l in range(3):
        want[f"room_color.planes{l}"] = e[l]["planes"].tobytes()
    for l in (0, 1):
        want[f"room_color.gradients{l}"] = fc.view_gradients(l).tobytes()
        px = jm.pixels(**fc.loop_args(l))
        want[f"l{l}.sums"] = gicp_model.canonical(px["terms"]).tobytes() + np.int64((px["pixel"] >= 0).sum()).tobytes()
        want[f"l{l}.pairs"] = px["pixel"].tobytes() + px["dist"].tobytes()
    h = fc.expected("5x7_hole", 0)
    want["5x7_hole.view"] = np.int32([[h["n_valid"]], [h["n_no_normal"]]]).tobytes() + h["planes"].tobytes()
    return want
