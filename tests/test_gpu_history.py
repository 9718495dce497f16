"""The history matrix on the device (tests/history_cases.py): for fixed inputs and fixed settings every public result of
a context is the same bytes whatever the context did before.

Every probe of history_cases.PROBES runs on the probe scene P
  - on fresh contexts and twice on one (test_probe_is_repeatable),
  - against the independent models the suite owns (test_fresh_probe_equals_its_model): bit for bit wherever the
    feature's own test claims bit equality, at that test's tolerance where it claims one,
  - after every history of history_cases.HISTORIES -- every probe on the large scene Q and on the tiny scene S, and the
    documented early paths -- in a fixed order and then in the reverse order, on the one context that ran the history
    (test_history_then_probe): the earlier probes are history for the later ones,
  - in the chain Q, S, P, S, Q, P (test_shrink_grow_chain).
Bytes or nothing: no tolerance, no retry."""
import numpy as np
import pytest

import history_cases as hc
from icp_slam_prototype_amd import binding

pytestmark = pytest.mark.gpu

B = binding


@pytest.fixture(scope="module", autouse=True)
def torch_device_first():
    """The batch probe hands device memory of torch's to the library, and the communicator history loads the RCCL that
    torch ships: torch's runtime has to open the device before the first context does (as it has in a run of the
    whole suite, where tests/test_gpu_batch.py comes first); the other way round torch finds no device."""
    import torch

    torch.cuda.init()
    torch.zeros(1).cuda()
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def fresh(torch_device_first):
    """every probe on P, each on a context that has done nothing else; computed once and left unchanged"""
    s = hc.scene("P")
    out = {}
    for name, probe in hc.PROBES.items():
        with B.Context(0) as c:
            out[name] = probe(c, s)
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


@pytest.mark.parametrize("probe", hc.PROBE_ORDER)
def test_probe_is_repeatable(fresh, probe):
    s = hc.scene("P")
    with B.Context(0) as c:
        first = hc.PROBES[probe](c, s)
        second = hc.PROBES[probe](c, s)
    bad = differences(first, fresh[probe], probe + " on a second fresh context") + \
        differences(second, fresh[probe], probe + " run twice on one context")
    assert not bad, "\n".join(bad)
    assert len(fresh[probe]) >= 4 and all(isinstance(v, bytes) for v in fresh[probe].values())


def same_as_model(got, want, probe):
    """every key the model gives, bit for bit"""
    bad = []
    for k, v in want.items():
        if k in ("facts", "rows", "want"):
            continue
        assert k in got, (probe, k)
        g, v = got[k], np.asarray(v)
        if g.dtype != v.dtype and g.dtype.kind in "iub" and v.dtype.kind in "iub":  # (an integer of another width)
            assert np.array_equal(v, v.astype(g.dtype)), (probe, k)
            v = v.astype(g.dtype)
        w = hc.blob(v)
        if g != w:
            bad.append(f"{probe}[{k}] against its model: {hc.first_difference(g, w)}")
    return bad


def align_reference(s, flavour):
    """the probe's two runs through the exact kernel and the host loop (as soak_cases.soak_align compares them)"""
    with B.Context(0) as c:
        kw = hc.install_flavour(c, s, flavour)
        kw.update(nn_mode=B.NN_EXACT, host_loop=1)
        return hc.align_runs(c, s, flavour, kw)


@pytest.mark.parametrize("probe", [p for p in hc.PROBE_ORDER])
def test_fresh_probe_equals_its_model(fresh, probe, oracle):
    s = hc.scene("P")
    got = fresh[probe]
    given = {k: hc.unblob(got[k]) for k in ("target_normals", "source_normals", "gradients") if k in got}
    bad = []
    if probe == "batch":
        # the lock-step pairs against the same pairs one by one (soak_cases.soak_batch's comparison)
        with B.Context(0) as c:
            for b, (src, tgt) in enumerate(hc.batch_pairs(s)):
                c.set_target(tgt)
                c.set_source(src)
                T, st, rc = c.align(**hc.BATCH_ALIGN)
                idx, dist = c.get_associations()
                for tag in ("batch", "device"):
                    assert hc.unblob(got[tag + ".T"])[b].tobytes() == T.tobytes(), (tag, b)
                    assert hc.unblob(got[f"{tag}.{b}.stats"])[:3].tolist() == [st.iterations, st.status, st.final_pairs], (tag, b)
                assert got[f"batch.{b}.idx"] == idx.tobytes() and got[f"batch.{b}.dist"] == dist.tobytes(), b
        return
    want = hc.MODELS[probe](s, oracle, given)
    bad += same_as_model(got, want, probe)
    if probe == "fpfh":
        # the large run's valid hypotheses do cross a scoring chunk of SCORE_MAX_POSES (global.rest: rc, hypothesis,
        # inliers, n_valid, n_matches), and the host model counted the same number
        rest = hc.unblob(got["global.rest"])
        assert rest[3] > B.SCORE_MAX_POSES and rest[3] == want["facts"]["large_n_valid"] and rest[0] == B.OK, rest
    if probe.startswith("align_"):
        # the grid scan and the device loop against the exact kernel and the host loop: transform, status, iterations,
        # pair count, mse, associations, moved source (soak_cases.soak_align's list), for both runs
        ref = align_reference(s, probe[len("align_"):])
        for run in ("fixed", "exit"):
            for k in ("T", "rc", "mse", "idx", "dist", "source"):
                if got[f"{run}.{k}"] != ref[f"{run}.{k}"]:
                    bad.append(f"{probe}[{run}.{k}] against exact kernel + host loop: "
                               f"{hc.first_difference(got[f'{run}.{k}'], ref[f'{run}.{k}'])}")
            a, b = hc.unblob(got[run + ".stats"]), hc.unblob(ref[run + ".stats"])
            if a[:3].tolist() != b[:3].tolist():
                bad.append(f"{probe}[{run}.stats]: {a[:3]} against {b[:3]}")
        assert hc.unblob(got["fixed.stats"])[0] == hc.FIXED_ITERATIONS
        assert 1 <= hc.unblob(got["exit.stats"])[0] < 2 * hc.FIXED_ITERATIONS  # (the threshold did end the second run)
    if probe == "normals":
        # the normals themselves: tests/test_gpu_normals.py::_check, at its own tolerance (1e-6 rad on the points it
        # compares; count and moments bit for bit), on a context of its own -- which must return the probe's bytes
        import test_gpu_normals as tn

        with B.Context(0) as c:
            _, lib = tn._check(c, s["target"], hc.radius(s), 5, s["viewpoint"], name="history P")
        assert lib["normals"].tobytes() == got["target_normals"] and lib["curvature"].tobytes() == got["curvature"]
        assert hc.unblob(got["n"]).tolist() == [lib["n"], lib["n_valid"]]
    if probe == "score":
        import score_model as sm

        sums, inl = hc.unblob(got["sums"]), hc.unblob(got["inliers"])
        info = hc.unblob(got["information"])
        for k, row in want["rows"].items():  # tests/test_gpu_score.py::check_model's comparison, per pose
            assert inl[k] == row["inliers"] and sums[k].tobytes() == row["sums"].tobytes(), k
            assert info[k].tobytes() == sm.information(row["sums"], row["inliers"]).tobytes(), k
    if probe == "posegraph":
        # tests/test_gpu_posegraph.py::_compare: poses and cost within 16 x the graph's sensitivity to summation order
        import posegraph_cases as pc

        P = hc.unblob(got["poses"]).reshape(-1, 4, 4)
        cost = float(hc.unblob(got["result.float"])[1])
        m = want["want"]
        bound = 16 * pc.s_graph(hc.PG_CASE)  # (case A: 0 -- the model's poses and cost exactly)
        dp = float(np.abs(P - m["poses"]).max())
        dc = abs(cost - m["final_cost"]) / m["final_cost"]
        print(f"posegraph: pose {dp:.3e}, relative cost {dc:.3e}, bound {bound:.3e}")
        assert dp <= bound and dc <= bound
    assert not bad, "\n".join(bad)


def probes_against_fresh(ctx, fresh, order, tag):
    s = hc.scene("P")
    bad = []
    for name in order:
        bad += differences(hc.PROBES[name](ctx, s), fresh[name], f"{tag}: probe {name}")
    return bad


@pytest.mark.parametrize("history", list(hc.HISTORIES))
def test_history_then_probe(fresh, history):
    with B.Context(0) as c:
        hc.HISTORIES[history](c)
        bad = probes_against_fresh(c, fresh, hc.PROBE_ORDER, f"after history {history}")
        bad += probes_against_fresh(c, fresh, hc.PROBE_ORDER[::-1], f"after history {history} and every probe, reversed order")
    assert not bad, "\n".join(bad[:40])


@pytest.mark.parametrize("history", list(hc.EARLY))
def test_early_history_takes_its_path(history):
    """the early-path histories do end where their names say (what the history saw against what the header defines)"""
    with B.Context(0) as c:
        facts = hc.EARLY[history](c)
    assert facts, history
    wrong = [(label, got, want) for label, got, want in facts if got != want]
    assert not wrong, wrong


def test_shrink_grow_chain(fresh):
    bad = []
    with B.Context(0) as c:
        for k, name in enumerate("QSPSQP"):
            s = hc.scene(name)
            for probe in hc.CHAIN_PROBES:
                got = hc.PROBES[probe](c, s)  # (to its end on every scene: a refusal is raised)
                if name == "P":
                    bad += differences(got, fresh[probe], f"chain step {k} ({'QSPSQP'[:k + 1]}): probe {probe}")
    assert not bad, "\n".join(bad[:40])
