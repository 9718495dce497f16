"""The signed updates of the TSDF volume (K30) held to INTEGRATION.md's threading row as
tests/test_gpu_frame_view_threads.py holds the frame view: the script of tests/tsdf_apply_thread_cases.py on 8 threads at
once, each thread on contexts of its own, against the same script run alone on a fresh context, byte for byte.  No number
here is a tolerance; the join time-out is the only time.  Nothing is repeated until it fails: 8 threads, 2 rounds each, a
fresh context per round and one context reused for both by the odd threads -- whose second round runs every call on a
context that has held volumes and frame stacks of other shapes."""
import threading
import traceback

import pytest

import tsdf_apply_thread_cases as atc
from icp_slam_prototype_amd import binding

pytestmark = pytest.mark.gpu

T, ROUNDS, TIMEOUT = 8, 2, 120.0


@pytest.fixture(scope="module")
def serial():
    runs = []
    for _ in range(2):
        with binding.Context(0) as c:
            runs.append(atc.script(c))
    return runs


def test_script_alone_is_repeatable_and_gives_the_models_bytes(serial):
    assert atc.first_difference(*serial) is None
    got = dict(serial[0])
    assert len(got) == len(serial[0]) and all(len(v) > 0 for v in got.values())
    for label, want in atc.model_outputs().items():
        assert got[label] == want, label
    assert "deintegrate" in got and "refuse" in got


def test_a_reused_context_gives_a_fresh_contexts_bytes(serial):
    with binding.Context(0) as c:
        first, second = atc.script(c), atc.script(c)
    assert atc.first_difference(first, serial[0]) is None and atc.first_difference(second, serial[0]) is None


def test_eight_threads_apply_signed_updates_concurrently(serial):
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
                        results[k].append(atc.script(reused))
                    else:
                        with binding.Context(0) as c:
                            results[k].append(atc.script(c))
            finally:
                if reused is not None:
                    reused.close()
        except threading.BrokenBarrierError:
            pass
        except BaseException as e:  # noqa: BLE001 (reported below)
            errors[k] = f"{type(e).__name__}: {e}\n{traceback.format_exc()}"
            stop.set()
            barrier.abort()

    threads = [threading.Thread(target=body, args=(k,), daemon=True, name=f"icpk-tsdf-apply-{k}") for k in range(T)]
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
            d = atc.first_difference(got, serial[0])
            assert d is None, f"thread {k}, round {i}: output {d[0]} differs from the serial run at byte {d[1]}"
