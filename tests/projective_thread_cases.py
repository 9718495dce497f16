"""The projective family (K25) as a thread script, in the style of tests/pyramid_thread_cases.py: one function that makes
every call of the family on a context it is handed and returns its outputs as a list of (label, bytes).  tests/
test_gpu_projective_threads.py runs it alone on fresh contexts, then on eight threads at once, each thread on contexts
of its own, and compares byte for byte.

The calls: on the room at level 0 and at level 1 (the view's shape differs) the 10-iteration loop with its trace, one
reduction and the per-pixel association; the normal gate's reduction (the other kernel); a loop that stops at once."""
import numpy as np

import projective_cases as pc
from icp_slam_prototype_amd import binding, depth

from pyramid_thread_cases import first_difference  # noqa: F401 (the comparison the thread test uses)


def script(ctx):
    """Every call of the family, on `ctx`.  Returns [(label, bytes)]."""
    out = []
    for name in pc.LOOP_CASES:
        c = pc.case(name)
        p = pc.device_setup(ctx, name, depth, binding)
        pose, res = binding.align_projective(ctx, c["estimate"], p)
        out.append((f"{name}.pose", pose.tobytes() + bytes(res)))
        for k, t in enumerate(binding.projective_trace(ctx)):
            out.append((f"{name}.trace{k}", t["pose"].tobytes() + t["sums"].tobytes() + np.int64([t["count"], t["status"]]).tobytes()))
        sums, count = binding.projective_reduce(ctx, c["estimate"], p)
        out.append((f"{name}.sums", sums.tobytes() + np.int64(count).tobytes()))
        pixel, dist = binding.projective_associate(ctx, c["estimate"], p)
        out.append((f"{name}.pairs", pixel.tobytes() + dist.tobytes()))
    c = pc.case("normal_gate")
    sums, count = binding.projective_reduce(ctx, c["estimate"], pc.device_setup(ctx, "normal_gate", depth, binding))
    out.append(("normal_gate.sums", sums.tobytes() + np.int64(count).tobytes()))
    c = pc.case("plane")
    pose, res = binding.align_projective(ctx, c["estimate"], pc.device_setup(ctx, "plane", depth, binding))
    out.append(("plane.pose", pose.tobytes() + bytes(res)))
    return out


def model_outputs():
    """{label: bytes} of the outputs the model states: the sums and pairs at the cases' estimates"""
    want = {}
    for name in pc.LOOP_CASES + ("normal_gate",):
        e = pc.expected(name)
        want[f"{name}.sums"] = e["sums"].tobytes() + np.int64(e["count"]).tobytes()
        if name in pc.LOOP_CASES:
            want[f"{name}.pairs"] = e["pixel"].tobytes() + e["dist"].tobytes()
    return want
