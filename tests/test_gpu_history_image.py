"""The history matrix of the image and volume families on the device (tests/history_image_cases.py): for fixed inputs
and fixed settings every public result of the functions over a context -- K22 to K31 -- is the same bytes whatever the
context did before.

Every probe of history_image_cases.PROBES (nine families -- K27's fern probe is left out, see history_image_cases.py
-- and history_cases' `tsdf` and `frontend`, which share the volume and the image buffers with them) runs on the probe
scene P
  - on fresh contexts and twice on one (test_probe_is_repeatable),
  - against the numpy models the suite owns, bit for bit (test_fresh_probe_equals_its_model),
  - after every history of history_image_cases.HISTORIES -- every probe on the large scene Q with its larger volume
    and on the tiny scene S with its 60 voxels, three of history_cases' probes on Q, and the early and left-over
    states -- in a fixed order and then in the reverse order, on the one context that ran the history
    (test_history_then_probe),
  - in the chain Q, S, P, S, Q, P, the nine new probes with each scene's own volume, `tsdf` with history_cases' one
    volume throughout (test_shrink_grow_chain).
test_a_probe_that_installs_less_is_noticed shows that the comparison sees leaked state: three probes that leave one
installing call out differ from the fresh bytes after the history that leaves the matching state.
Bytes or nothing: no tolerance, no retry."""
import numpy as np
import pytest

import history_cases as hc
import history_image_cases as hi
from icp_slam_prototype_amd import binding

pytestmark = pytest.mark.gpu

B = binding


@pytest.fixture(scope="module")
def fresh():
    """every probe on P, each on a context that has done nothing else; computed once and left unchanged"""
    s = hi.scene("P")
    out = {}
    for name in hi.PROBE_ORDER:
        with B.Context(0) as c:
            out[name] = hi.PROBES[name](c, s)
    return out


def differences(got, want, probe):
    """the keys of one probe's result that differ from the fresh bytes, each with its first difference"""
    bad = []
    if got.keys() != want.keys():
        bad.append(f"{probe}: keys differ: {sorted(set(got) ^ set(want))}")
    for k in want:
        if k in got and got[k] != want[k]:
            bad.append(f"{probe}[{k}]: {hc.first_difference(got[k], want[k])}")
    return bad


@pytest.mark.parametrize("probe", hi.PROBE_ORDER)
def test_probe_is_repeatable(fresh, probe):
    s = hi.scene("P")
    with B.Context(0) as c:
        first = hi.PROBES[probe](c, s)
        second = hi.PROBES[probe](c, s)
    bad = differences(first, fresh[probe], probe + " on a second fresh context") + \
        differences(second, fresh[probe], probe + " run twice on one context")
    assert not bad, "\n".join(bad)
    assert len(fresh[probe]) >= 4 and all(isinstance(v, bytes) for v in fresh[probe].values())


def same_as_model(got, want, probe):
    """every key the model gives, bit for bit.  `X.trace0_pose / _sums / _count`: the first evaluated iteration of the
    loop X, whose pose is the estimate handed in and whose sums are the reduction's at that estimate."""
    bad = []
    for k, v in want.items():
        if k == "facts":
            continue
        v = np.asarray(v)
        if ".trace0_" in k:
            loop, field = k.split(".trace0_")
            assert hc.unblob(got[loop + ".trace_n"]) >= 1, (probe, k)
            g = hc.blob(hc.unblob(got[f"{loop}.trace_{field}"])[0])
        else:
            assert k in got, (probe, k)
            g = got[k]
        if g.dtype != v.dtype and g.dtype.kind in "iub" and v.dtype.kind in "iub":  # (an integer of another width)
            assert np.array_equal(v, v.astype(g.dtype)), (probe, k)
            v = v.astype(g.dtype)
        w = hc.blob(v)
        if g != w:
            bad.append(f"{probe}[{k}] against its model: {hc.first_difference(g, w)}")
    return bad


LOOPS = {"projective": ("l0.align", "l1.align"), "projective_colored": ("l0.colored_align", "l1.colored_align"),
         "frame_view": ("view.l0.align", "view.l1.align", "view.l0.colored_align", "view.l1.colored_align"),
         "sdf": ("fused.l0.align", "fused.l1.align", "shifted.l0.align")}


@pytest.mark.parametrize("probe", hi.PROBE_ORDER)
def test_fresh_probe_equals_its_model(fresh, probe, oracle):
    s = hi.scene("P")
    got = fresh[probe]
    want = hi.MODELS[probe](s, oracle, {})
    bad = same_as_model(got, want, probe)
    for loop in LOOPS.get(probe, ()):
        # the loop did run on P: every iteration evaluated, none stopped for want of pairs (tests/test_history_image_host.py
        # holds the first iteration's count on the models), and the trace is the loop's own
        status, iterations = hc.unblob(got[loop + ".result"])
        n = int(hc.unblob(got[loop + ".trace_n"]).reshape(-1)[0])
        assert status == B.OK and iterations == n == hi.LOOP_ITERATIONS, (loop, status, iterations, n)
        assert (hc.unblob(got[loop + ".trace_status"]) == B.OK).all() and (hc.unblob(got[loop + ".trace_count"]) >= 6).all(), loop
    assert not bad, "\n".join(bad)
    assert len([k for k in want if k != "facts"]) >= 3, probe


def probes_against_fresh(ctx, fresh, order, tag):
    s = hi.scene("P")
    bad = []
    for name in order:
        bad += differences(hi.PROBES[name](ctx, s), fresh[name], f"{tag}: probe {name}")
    return bad


@pytest.mark.parametrize("history", list(hi.HISTORIES))
def test_history_then_probe(fresh, history):
    with B.Context(0) as c:
        hi.HISTORIES[history](c)
        bad = probes_against_fresh(c, fresh, hi.PROBE_ORDER, f"after history {history}")
        bad += probes_against_fresh(c, fresh, hi.PROBE_ORDER[::-1], f"after history {history} and every probe, reversed order")
    assert not bad, "\n".join(bad[:40])


@pytest.mark.parametrize("history", list(hi.EARLY))
def test_early_history_takes_its_path(history):
    """the early-path histories do end where their names say (what the history saw against what the header defines)"""
    with B.Context(0) as c:
        facts = hi.EARLY[history](c)
    assert facts, history
    wrong = [(label, got, want) for label, got, want in facts if got != want]
    assert not wrong, wrong


def test_shrink_grow_chain(fresh):
    bad = []
    with B.Context(0) as c:
        for k, name in enumerate(hi.CHAIN):
            s = hi.scene(name)
            for probe in hi.PROBE_ORDER:
                # (to its end on every scene: a refusal is raised.  The nine new probes create the scene's own volume;
                # history_cases' `tsdf` and `frontend` are unchanged and `tsdf` always creates history_cases.TSDF_VOLUME)
                got = hi.PROBES[probe](c, s)
                if name == "P":
                    bad += differences(got, fresh[probe], f"chain step {k} ({hi.CHAIN[:k + 1]}): probe {probe}")
    assert not bad, "\n".join(bad[:40])


# ---- probes that install less -----------------------------------------------------------------------------------------
# Each is one of the probes above with ONE installing call left out, so that what it reads there is whatever the
# context's past left.  All three run after history_image_cases.early_selector_left_live, which leaves on P's own shapes
# (40 x 60, three levels): the selector at ICPK_VIEW_FRAME, level 0; a live coloured frame view of P's target frame; and
# that frame's pyramid resident with its intensity levels.
#
# Every call in them is a valid public call with defined behaviour, and nothing is read outside a live buffer:
#   - under ICPK_VIEW_FRAME the projective kernels are handed the snapshot's own planes with the snapshot's own shape,
#     fx / 2^level and pose (include/icpk.h, icpk_projective_set_view); the snapshot is live -- the history does not
#     release it -- and no pyramid build touches it;
#   - the SDF and frame view calls read the resident pyramid through its own recorded shapes (pyr_rows / pyr_cols), and
#     the binding sizes every host array from icpk_depth_pyramid_shape and icpk_frame_view_shape, not from the scene;
#   - the history's pyramid has P's shape and three levels, so every level the variants ask for exists.
# On a fresh context the first variant is the probe itself (ICPK_VIEW_RAYCAST is the default), and the other two are
# refused with ICPK_E_NOT_SET (no pyramid): that is asserted as well.
def projective_without_set_view(ctx, s):
    """probe_projective without its projective_set_view"""
    hc.settings(ctx)
    out = {}
    hi.volume(ctx, s)
    hi.fuse(ctx, s)
    out["raycast.counts"] = hc.blob(np.array(hi.raycast(ctx, s, s["pose_src"]), np.int32))
    out["raycast.maps"] = hc.blob(hi._maps(ctx))
    hi.pyramid(ctx, s, "src")
    hi._projective_calls(ctx, s, out, hi.drift(s["pose_src"]))
    return out


def sdf_without_pyramid(ctx, s):
    """probe_sdf without rebuilding the pyramid"""
    hi.settings(ctx)
    out = {}
    hi.volume(ctx, s)
    hi.fuse(ctx, s)
    hi._sdf_body(ctx, s, out)
    return out


def frame_view_without_plain_pyramid(ctx, s):
    """probe_frame_view without the pyramid build of its uncoloured view: the build is the one call that takes the
    intensity levels away (set_pyramid_intensity has no inverse), so the uncoloured view's "no intensity" is installed
    by it"""
    hi.settings(ctx)
    out = {}
    hi._plain_view(ctx, s, out)
    hi._colored_view(ctx, s, out)
    return out


# variant -> (the probe it is cut from, the keys that must differ after the history, what a fresh context answers)
INSTALLS_LESS = {
    "projective_without_set_view": (projective_without_set_view, "projective", ("l0.pixel", "l0.sums", "l1.pixel"), None),
    "sdf_without_pyramid": (sdf_without_pyramid, "sdf", ("fused.l0.cell", "fused.l0.sums", "shifted.l0.cell"), B.E_NOT_SET),
    "frame_view_without_plain_pyramid": (frame_view_without_plain_pyramid, "frame_view", ("plain.planes0", "plain.gradients_rc"),
                                         B.E_NOT_SET),
}


@pytest.mark.parametrize("variant", list(INSTALLS_LESS))
def test_a_probe_that_installs_less_is_noticed(fresh, variant):
    fn, probe, keys, fresh_refusal = INSTALLS_LESS[variant]
    s = hi.scene("P")
    with B.Context(0) as c:  # on a fresh context: the probe's own bytes, or the refusal of a call that finds no pyramid
        if fresh_refusal is None:
            assert not differences(fn(c, s), fresh[probe], variant + " on a fresh context")
        else:
            with pytest.raises(B.IcpkError) as e:
                fn(c, s)
            assert e.value.code == fresh_refusal
    with B.Context(0) as c:
        facts = hi.early_selector_left_live(c)
        assert all(got == want for _, got, want in facts), facts
        got = fn(c, s)
        # ... and the complete probe, straight after on the same context, is the fresh bytes again
        bad = differences(hi.PROBES[probe](c, s), fresh[probe], f"{probe} after {variant}")
    assert got.keys() == fresh[probe].keys()
    differing = {k for k in got if got[k] != fresh[probe][k]}
    print(variant, "differs in", sorted(differing))
    assert set(keys) <= differing, (variant, sorted(differing))
    assert not bad, "\n".join(bad)
