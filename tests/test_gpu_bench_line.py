"""bench.py --gpus 1 as it is run for every change: the plain line (headline only, exactly --steps timed steps) and
--dump-outputs (what the last timed step handed its caller), checked against the same alignment made through the
binding in this process, bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from icp_slam_prototype_amd import binding, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "iter/s" and d["value"] > 0
    assert d["higher_is_better"] is True and d["dtype"] and d["metric"] and d["ms_per_step"] > 0
    assert d["timed_blocks"]["blocks"] == 1 and len(d["timed_blocks"]["ms_each"]) == 1
    # value and ms_per_step describe the same 3 steps of 20 iterations
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - 20) < 1e-6 * 20
    for k in ("cpu_baseline", "frame_batch", "extra", "roofline", "stage_ms_per_step", "pcie_inclusive_iter_s"):
        assert k not in d, k  # --full only

    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(got) == {"transform", "stats", "return_code", "aligned_source", "nn_index", "nn_distance"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20

    p = synth.kinect_pair(480, 640, valid=0.30, seed=2)  # bench.py's default workload
    with binding.Context(0) as ctx:
        ctx.set_target(p["target"])
        ctx.set_source(p["source"])
        T, st, rc = ctx.align(max_iterations=20, fixed_iterations=1, max_nn_dist=0.75, solve=binding.SOLVE_REFERENCE,
                              nn_mode=binding.NN_GRID)
        idx, dist = ctx.get_associations()
        src = ctx.get_source()
    assert np.array_equal(got["transform"].view(np.uint32), T.view(np.uint32))
    assert got["stats"].tolist() == [[st.iterations, st.status, st.final_pairs, float(np.float32(st.final_mse))]]
    assert got["stats"][0, 0] == 20 and got["return_code"].tolist() == [rc]
    assert np.array_equal(got["nn_index"], idx.astype(np.float64))
    assert np.array_equal(got["nn_distance"].view(np.uint32), dist.view(np.uint32))
    assert np.array_equal(got["aligned_source"].view(np.uint32), src.view(np.uint32))
