"""The fern family (K27) held to INTEGRATION.md's threading row as tests/test_gpu_projective_threads.py holds the
projective one: 8 threads at once, each harvesting the scene's first frames into a database on a context of its own and
querying it, against the same script run alone on a fresh context, byte for byte.  No number here is a tolerance; the
join time-out is the only time.  Nothing is repeated until it fails: 8 threads, 2 rounds each, a fresh context per round
and one context reused for both by the odd threads."""
import threading
import traceback

import pytest

import fern_model as fm
from icp_slam_prototype_amd import binding, depth

pytestmark = pytest.mark.gpu

T, ROUNDS, TIMEOUT, COUNT = 8, 2, 120.0, 12


def script(c):
    """[(label, bytes)]: the harvest of the first COUNT frames, the database, and three queries"""
    s = fm.scene()
    pp = depth.pyramid_params(levels=3)
    binding.fern_create(c, 30, 40)
    out = []
    for i in range(COUNT):
        depth.build_pyramid(c, s["frames"][i], pp)
        r = binding.fern_process(c, s["poses"][i], 3)
        out.append((f"frame{i}", r["index"].tobytes() + r["diss"].tobytes() + f"{r['valid']},{r['added']}".encode()))
    for j in range(binding.fern_count(c)):
        code, pose = binding.fern_keyframe(c, j)
        out.append((f"keyframe{j}", code.tobytes() + pose.tobytes()))
    for i in (2, 7, 30):
        depth.build_pyramid(c, s["queries"][i], pp)
        code, V = binding.fern_encode(c)
        idx, d = binding.fern_query(c, 8)
        out.append((f"query{i}", code.tobytes() + idx.tobytes() + d.tobytes() + str(V).encode()))
    return out


def first_difference(a, b):
    if [l for l, _ in a] != [l for l, _ in b]:
        return "labels", 0
    for (label, x), (_, y) in zip(a, b):
        if x != y:
            return label, next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
    return None


@pytest.fixture(scope="module")
def serial():
    runs = []
    for _ in range(2):
        with binding.Context(0) as c:
            runs.append(script(c))
    return runs


def test_script_alone_is_repeatable_and_gives_the_models_database(serial):
    assert first_difference(*serial) is None
    got = dict(serial[0])
    db, want = fm.scene_harvest(count=COUNT)
    assert [l for l in got if l.startswith("keyframe")] == [f"keyframe{j}" for j in range(len(db.codes))] and len(db.codes) == 3
    for j, (code, pose) in enumerate(zip(db.codes, db.poses)):
        assert got[f"keyframe{j}"] == code.tobytes() + pose.tobytes()
    for i, w in enumerate(want):
        assert got[f"frame{i}"] == w["index"].tobytes() + w["diss"].tobytes() + f"{w['valid']},{w['added']}".encode()
    for i in (2, 7, 30):
        w = db.process(fm.scene_levels("queries")[i], None, 8)
        assert got[f"query{i}"] == w["code"].tobytes() + w["index"].tobytes() + w["diss"].tobytes() + str(w["valid"]).encode()


def test_eight_threads_harvest_and_query_concurrently(serial):
    stop, barrier = threading.Event(), threading.Barrier(T)
    results, errors = [[] for _ in range(T)], [None] * T

    def body(k):
        try:
            barrier.wait(timeout=60)
            reused = binding.Context(0) if k % 2 else None
            try:
                for _ in range(ROUNDS):
                    if stop.is_set():
                        return
                    if reused is not None:
                        results[k].append(script(reused))
                    else:
                        with binding.Context(0) as c:
                            results[k].append(script(c))
            finally:
                if reused is not None:
                    reused.close()
        except threading.BrokenBarrierError:
            pass
        except BaseException as e:  # noqa: BLE001 (reported below)
            errors[k] = f"{type(e).__name__}: {e}\n{traceback.format_exc()}"
            stop.set()
            barrier.abort()

    threads = [threading.Thread(target=body, args=(k,), daemon=True, name=f"icpk-fern-{k}") for k in range(T)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(TIMEOUT)
    hung = [t.name for t in threads if t.is_alive()]
    if hung:
        stop.set()
        pytest.fail(f"still running after {TIMEOUT:.0f} s: {hung}")
    assert not any(errors), "\n".join(f"thread {k}: {e}" for k, e in enumerate(errors) if e)
    for k in range(T):
        assert len(results[k]) == ROUNDS, k
        for i, got in enumerate(results[k]):
            d = first_difference(got, serial[0])
            assert d is None, f"thread {k}, round {i}: output {d[0]} differs from the serial run at byte {d[1]}"
