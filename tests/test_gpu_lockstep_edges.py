"""Lock-step pairs (icpk_align_batch, icpk_align_batch_device) at the geometry where grids collapse or clamp, held to
brute force: the exact kernel (literal arithmetic of icp.cpp:566-620 per pair, no spatial index) driven by the host loop
on a plain context, and the CPU oracle's brute-force scan.  tests/test_gpu_batch.py only asserts batch == single on
well-behaved pairs, which cannot see a defect the batch and the single grid path share.

/root/reference does not exist on the GPU box: nothing here reads it.
"""
import numpy as np
import pytest

from icp_slam_prototype_amd import binding, synth
from tests.test_gpu_batch import _Hip

pytestmark = pytest.mark.gpu

GRID_MAX_CELLS_SLOT = 1 << 21  # icpk_internal.h: a frame-batch slot's cell table (a plain context's: 2^23)


def grid_cells_f32(tgt, ppc=8.0, xdiv=4):
    """(nx, ny, nz) grid_info_body asks for before it grows the cell edge to fit the table: its float32 arithmetic
    restated (extent of the finite points, h = sqrt(ppc * area / n), at least emax / 1023; cells xdiv times finer
    along x)."""
    f = np.float32
    fin = tgt[:, np.isfinite(tgt).all(0)]
    ext = [f(fin[c].max()) - f(fin[c].min()) for c in range(3)]
    emax = max(ext)
    area = ext[0] * ext[1] + ext[1] * ext[2] + ext[2] * ext[0]
    h = np.sqrt(f(ppc) * area / f(tgt.shape[1]), dtype=np.float32)
    h = max(h, f(emax / f(1023)))
    hx = f(h / f(xdiv))
    return int(ext[0] / hx) + 1, int(ext[1] / h) + 1, int(ext[2] / h) + 1


def adversarial_pairs():
    """(name, source, target): the degenerate targets of test_grid_degenerate_target_shapes, axis-normal planes,
    non-finite targets, far queries, a blob inside one cell, lopsided sizes, an empty source, a volumetric target that
    overflows a slot's cell table, a min_pairs fallback and a pair that exits early on the threshold."""
    rng = np.random.default_rng(2024)
    src = (rng.uniform(-1, 1, (3, 3000)) + 5).astype(np.float32)
    out = []
    out.append(("identical", src, np.tile(np.array([[5.0], [5.5], [4.5]], np.float32), (1, 700))))
    out.append(("collinear", src,
                np.stack([np.linspace(4, 6, 5000), np.full(5000, 5.0), np.full(5000, 5.0)]).astype(np.float32)))
    for axis in range(3):  # planes normal to x, y, z
        pl = rng.uniform(4, 6, (3, 20000))
        pl[axis] = 5.25
        out.append((f"plane{axis}", src, pl.astype(np.float32)))
    out.append(("single", src, np.array([[4.0], [5.0], [6.0]], np.float32)))
    out.append(("clusters500m", src, np.concatenate([rng.normal(0, 0.01, (3, 4000)) + 5,
                                                     rng.normal(0, 0.01, (3, 4000)) + 500], 1).astype(np.float32)))
    nonfin = rng.uniform(4, 6, (3, 6000)).astype(np.float32)
    nonfin[0, 17], nonfin[1, 900], nonfin[2, 5999] = np.nan, np.inf, -np.inf
    out.append(("nonfinite", src, nonfin))
    out.append(("far_queries", rng.uniform(-50, 50, (3, 2000)).astype(np.float32),
                rng.uniform(0, 1, (3, 30000)).astype(np.float32)))
    centre = np.array([[0.5125], [0.51], [0.51]], np.float32)
    blob = np.concatenate([rng.uniform(0, 1, (3, 8000)), centre + rng.uniform(-0.002, 0.002, (3, 127))], 1)
    out.append(("blob127", (centre + rng.normal(0, 0.04, (3, 600))).astype(np.float32), blob.astype(np.float32)))
    for nq, nt in ((300, 500_000), (500_000, 300), (1, 200_000), (200_000, 1)):
        t = (rng.uniform(-2, 2, (3, nt)) + 5).astype(np.float32)
        out.append((f"lopsided{nq}x{nt}", (rng.uniform(-2, 2, (3, nq)) + 5).astype(np.float32), t))
    out.append(("empty_source", np.zeros((3, 0), np.float32), src))
    vol = rng.uniform(0, 1, (3, 450_000)).astype(np.float32)
    out.append(("volumetric", (vol[:, :2000] + rng.normal(0, 0.01, (3, 2000))).astype(np.float32), vol))
    a = synth.frustum_pair(800, seed=5, rot_deg=(0, 0.5, 0), shift=(0.002, 0, 0))
    far = a["source"] + np.float32(100)
    far[:, :2] = a["target"][:, :2] + np.float32(0.05)  # two queries within reach: < min_pairs = 3
    out.append(("fallback", far, a["target"]))
    out.append(("threshold_exit", a["source"], a["target"]))
    return out


def exact_single(ref, src, tgt, **kw):
    """the definition: exact kernel + host loop on a plain context"""
    ref.set_target(tgt)
    ref.set_source(src)
    T, st, rc = ref.align(nn_mode=binding.NN_EXACT, host_loop=1, **kw)
    idx, dist = ref.get_associations() if src.shape[1] else (np.zeros(0, np.int32), np.zeros(0, np.float32))
    return T.copy(), st, rc, idx, dist


def same(T, st, got_assoc, want, what):
    Tw, sw, rw, iw, dw = want
    assert np.array_equal(T.view(np.uint32), Tw.view(np.uint32)), f"{what}: T\n{T}\n{Tw}"
    assert (st.iterations, st.status, st.final_pairs) == (sw.iterations, sw.status, sw.final_pairs), what
    assert np.float32(st.final_mse).view(np.uint32) == np.float32(sw.final_mse).view(np.uint32), what
    if got_assoc is not None:
        assert np.array_equal(got_assoc[0], iw), f"{what}: indices"
        assert np.array_equal(got_assoc[1].view(np.uint32), dw.view(np.uint32)), f"{what}: distances"


RUNS = [  # both solve flavours, fixed iterations and the threshold exit; the fallback pair moves by last_translation
    dict(max_iterations=3, fixed_iterations=1, last_translation=np.array([0.01, -0.02, 0.03], np.float32)),
    dict(max_iterations=16, threshold=1e-4, solve=binding.SOLVE_KABSCH, last_translation=np.array([1, 2, 3], np.float32)),
]


@pytest.mark.parametrize("group,slices", [("16", "8"), ("4", "4")])
def test_lockstep_adversarial_pairs_against_brute_force(oracle, monkeypatch, group, slices):
    """Catches, per pair of a mixed group: a set-up workgroup past its pair's own count that does not leave (it would
    build into another pair's grid), a reduction that reads another pair's or an earlier group's partials, a slot whose
    clamped cell table loses candidates (the volumetric target asks for more than 4 x 2^21 cells: the slot's
    grid_info_body must grow the cell edge -- "efficiency only" in icpk_internal.h, checked here), a wrong row range
    of the collapsed grids (one cell, one row, one slab), and the group's per-pair loop control (fallback, early
    exit, an empty source sent down the single-pair path).  With 4 to a group the 18 pairs take 5 groups over the two
    alternating slot sets.  Every pair equals the exact kernel + host loop bit for bit (T, status, iterations, pairs,
    mse bits, associations), and the first sweep's associations equal the oracle's brute-force scan wherever
    nq * nt <= 1e9."""
    pairs = adversarial_pairs()
    names = [n for n, _, _ in pairs]
    nx, ny, nz = grid_cells_f32(pairs[names.index("volumetric")][2])
    assert nx * ny * nz > 4 * GRID_MAX_CELLS_SLOT  # (4 x 2^21 = 2^23: a plain context's table is outgrown too)
    assert len(pairs) > 16 and sum(s.shape[1] == 0 for _, s, _ in pairs) == 1
    plain = [(s, t) for _, s, t in pairs]

    # the first sweep (max_iterations = 0) against the CPU brute-force scan
    with binding.Context(0) as ref:
        first = [exact_single(ref, s, t, max_iterations=0) for s, t in plain]
    for (name, s, t), w in zip(pairs, first):
        if 0 < s.shape[1] * t.shape[1] <= 10 ** 9:
            oi, od = oracle.nn_bruteforce(s, t, threads=oracle.max_threads())
            assert np.array_equal(w[3], oi) and np.array_equal(w[4].view(np.uint32), od.view(np.uint32)), name

    monkeypatch.setenv("ICPK_BATCH_GROUP", group)  # (read at context creation)
    monkeypatch.setenv("ICPK_GRID_SLICES", slices)
    hip = _Hip()
    try:
        dev = [(hip.upload(s), s.shape[1], hip.upload(t), t.shape[1]) for s, t in plain]
        with binding.Context(0) as c:
            T, st, rc, assoc = c.align_batch(plain, associations=True, max_iterations=0)
            for k, name in enumerate(names):
                same(T[k], st[k], assoc[k] if plain[k][0].shape[1] else None, first[k], f"{name} first sweep")
            for kw in RUNS:
                with binding.Context(0) as ref:
                    want = [exact_single(ref, s, t, **kw) for s, t in plain]
                T, st, rc, assoc = c.align_batch(plain, associations=True, **kw)
                assert rc == max(w[2] for w in want)
                for k, name in enumerate(names):
                    same(T[k], st[k], assoc[k] if plain[k][0].shape[1] else None, want[k], f"{name} {kw}")
                Td, std, rcd = c.align_batch_device(dev, **kw)
                assert rcd == rc
                for k, name in enumerate(names):
                    same(Td[k], std[k], None, want[k], f"{name} device {kw}")
                got = dict(zip(names, st))
                assert got["fallback"].status == binding.W_TOO_FEW_PAIRS
                if "threshold" in kw:
                    assert got["threshold_exit"].iterations < kw["max_iterations"]  # left its group early
    finally:
        hip.free()


def test_row_range_of_the_grid_scan_at_its_largest(oracle, monkeypatch):
    """The worst case of nn_grid_body's row look-up ((rz, ry) from a float reciprocal and one correction step): a plane
    normal to x (nx = 1) whose y and z extents give ny = nz = 1024, the per-axis cap of grid_info_body (h >= emax /
    1023), so a query's cube can span 2^20 rows.  64 queries at x = +-50 make the unseeded first sweep scan all of
    them; queries on the plane scan few.  Catches a row decoded to the wrong (ry, rz) anywhere in [0, 2^20): a missed
    candidate, against the exact kernel and the oracle, on the single path and inside a lock-step group."""
    monkeypatch.setenv("ICPK_GRID_PPC", "0.25")  # (read at context creation)
    rng = np.random.default_rng(1024)
    n = 300_000
    e = np.float32(1023 / 1024)  # extent of y and z: emax / 1023 = 2^-10 exactly, so ext / h = 1023 exactly
    tgt = np.stack([np.full(n, 5.0), 4 + rng.uniform(0, 1, n) * e, 4 + rng.uniform(0, 1, n) * e]).astype(np.float32)
    tgt[1:, 0] = 4
    tgt[1:, 1] = 4 + e
    assert tgt[1].max() - tgt[1].min() == e and tgt[2].max() - tgt[2].min() == e
    assert grid_cells_f32(tgt, ppc=0.25) == (1, 1024, 1024)  # 2^20 cells: within both tables, no growth
    far = np.stack([np.where(np.arange(64) % 2, 55.0, -45.0), rng.uniform(4, 5, 64), rng.uniform(4, 5, 64)])
    near = tgt[:, rng.integers(0, n, 2000)] + rng.normal(0, 0.003, (3, 2000))
    src = np.concatenate([far, near], 1).astype(np.float32)
    oi, od = oracle.nn_bruteforce(src, tgt, threads=oracle.max_threads())
    kw = dict(max_iterations=2, fixed_iterations=1, solve=binding.SOLVE_KABSCH)
    with binding.Context(0) as c:
        c.set_target(tgt)
        c.set_source(src)
        ie, de = c.nn(binding.NN_EXACT)
        assert np.array_equal(ie, oi) and np.array_equal(de.view(np.uint32), od.view(np.uint32))
        c.reset_source()
        for _ in range(2):  # unseeded, then seeded
            ig, dg = c.nn(binding.NN_GRID)
            assert np.array_equal(ig, oi) and np.array_equal(dg.view(np.uint32), od.view(np.uint32))
        want = exact_single(c, src, tgt, **kw)
        c.reset_source()
        T, st, rc = c.align(**kw)
        same(T, st, c.get_associations(), want, "single")
    other = synth.frustum_pair(3000, seed=9)
    monkeypatch.setenv("ICPK_BATCH_GROUP", "2")
    with binding.Context(0) as c:
        T, st, rc, assoc = c.align_batch([(other["source"], other["target"]), (src, tgt)], associations=True,
                                         max_iterations=0)
        assert np.array_equal(assoc[1][0], oi) and np.array_equal(assoc[1][1].view(np.uint32), od.view(np.uint32))
        T, st, rc, assoc = c.align_batch([(other["source"], other["target"]), (src, tgt)], associations=True, **kw)
        same(T[1], st[1], assoc[1], want, "batch")
