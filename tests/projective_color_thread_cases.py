"""The coloured projective family (K26) as a thread script, in the style of tests/projective_thread_cases.py: one
function that makes every call of the family on a context it is handed and returns its outputs as a list of
(label, bytes).  tests/test_gpu_projective_color_threads.py runs it alone on fresh contexts, then on eight threads at
once, each thread on contexts of its own, and compares byte for byte.

The calls: on the room at level 0 and at level 1 the intensity pyramid, the view gradients with their kept sums, the
10-iteration coloured loop with its trace and one coloured reduction; the normal gate's coloured reduction (the other
instantiation); the wall's 20 iterations."""
import numpy as np

import projective_color_cases as kc
from icp_slam_prototype_amd import binding, depth

from pyramid_thread_cases import first_difference  # noqa: F401 (the comparison the thread test uses)


def script(ctx):
    """Every call of the family, on `ctx`.  Returns [(label, bytes)]."""
    out = []
    for name in kc.LOOP_CASES:
        c = kc.case(name)
        p = kc.device_setup(ctx, name, depth, binding, gradients=False)
        out.append((f"{name}.intensity", binding.pyramid_intensity(ctx, c["level"]).tobytes()))
        binding.raycast_color_gradients(ctx, c["radius"], c["min_neighbors"], keep_sums=True)
        g, S = binding.get_raycast_color_gradients(ctx, sums=True)
        out.append((f"{name}.gradients", g.tobytes()))
        out.append((f"{name}.gradient_sums", S.tobytes()))
        pose, res = binding.align_projective_colored(ctx, c["estimate"], p)
        out.append((f"{name}.pose", pose.tobytes() + bytes(res)))
        for k, t in enumerate(binding.projective_trace(ctx)):
            out.append((f"{name}.trace{k}", t["pose"].tobytes() + t["sums"].tobytes() + np.int64([t["count"], t["status"]]).tobytes()))
        sums, count = binding.projective_reduce_colored(ctx, c["estimate"], p)
        out.append((f"{name}.sums", sums.tobytes() + np.int64(count).tobytes()))
    c = kc.case("normal_gate")
    sums, count = binding.projective_reduce_colored(ctx, c["estimate"], kc.device_setup(ctx, "normal_gate", depth, binding))
    out.append(("normal_gate.sums", sums.tobytes() + np.int64(count).tobytes()))
    w = kc.wall()
    kc.create_volume(ctx, binding, "wall")
    ctx.tsdf_raycast(w["poses"][0], **kc.WALL_VIEW)
    binding.raycast_color_gradients(ctx, kc.WALL_RADIUS, kc.WALL_MIN_NB)
    depth.build_pyramid(ctx, w["frames"][1][0], depth.pyramid_params(levels=1), intensity=w["frames"][1][1])
    pose, res = binding.align_projective_colored(ctx, w["poses"][0], level=0, fx=kc.WALL_FX, cx=kc.WALL_CX,
                                                 max_iterations=kc.WALL_ITER, max_dist=kc.WALL_MAX_DIST)
    out.append(("wall.pose", pose.tobytes() + bytes(res)))
    return out


def model_outputs():
    """{label: bytes} of the outputs the model states"""
    want = {}
    for name in kc.LOOP_CASES + ("normal_gate",):
        e = kc.expected(name)
        want[f"{name}.sums"] = e["sums"].tobytes() + np.int64(e["count"]).tobytes()
        if name in kc.LOOP_CASES:
            want[f"{name}.intensity"] = kc.case(name)["level_intensity"].tobytes()
            want[f"{name}.gradients"] = kc.gradients_of(name).tobytes()
    return want
