"""The canonical reduction (include/icpk.h, ICPK_RED_*) against an EXACT sum, at the sizes where its geometry changes.

test_reduce_bit_exact_vs_oracle_canonical compares icpk_reduce with orc_sums_canonical, which restates the same tree:
a dropped block, a stale partial or a wrong grid stride that both share would pass it.  Here every sum is also held
to the correctly rounded exact sum of its terms (math.fsum over float64 terms), within the error bound of the tree:

    terms: b_r * a_c (a product of two floats: exact in float64), (double)(float)(a - b) (the float difference,
    exact once rounded to float), d, a, b: every term the kernel adds is exactly representable, so math.fsum of the
    float64 terms is the correctly rounded exact sum S.
    tree:  B = clamp(ceil(n / 256), 1, 256) blocks, P = 256 B lanes; lane g adds elements g, g + P, ... serially
    (L = ceil(n / P) terms: at most L - 1 roundings after the exact first add to +0.0), the 64-lane xor butterfly
    (6 adds), ((w0 + w1) + w2) + w3 (3 adds), and the same again over the 256 block slots (6 + 3 adds).  A term
    passes through at most k = L + 18 rounded adds (one spare), so |sum - S| <= k * 2^-53 * sum |t_i| (the gamma_k
    bound of a summation tree, gamma_k = k u / (1 - k u), with k u < 1e-14).

The sizes straddle the boundaries: n = 256 (one block, one pass), 65536 = RED_MAX_BLOCKS x RED_THREADS (the last
size with one pass), 65537 and up (the grid-stride loop's second pass), 1 000 003 (16 passes).
"""
import math

import numpy as np
import pytest

from icp_slam_prototype_amd import binding

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 511, 65535, 65536, 65537, 65536 + 255, 131073, 1_000_003]


def red_geometry(n):
    B = min(max((n + 255) // 256, 1), 256)
    return B, -(-n // (256 * B))


def chain(n):
    """k of the docstring: the most rounded adds any one term passes through"""
    return red_geometry(n)[1] + 18


@pytest.fixture(scope="module")
def ctx():
    from icp_slam_prototype_amd import build

    build.build()
    c = binding.Context(0)
    yield c
    c.close()


def cloud(n, seed, nt=3000):
    """targets about 5 m from the origin, queries near them (a few NaN ones from n >= 64 on)"""
    rng = np.random.default_rng(seed)
    tgt = (rng.uniform(-2, 2, (3, nt)) + 5).astype(np.float32)
    src = (tgt[:, rng.integers(0, nt, n)] + rng.normal(0, 0.03, (3, n))).astype(np.float32)
    return src, tgt


def nsum_terms(src, tgt, idx, acc):
    """the 19 per-pair terms of ICPK_NSUM for the accepted queries, each exact in float64"""
    a = src[:, acc]
    b = tgt[:, idx[acc]]
    ad, bd = a.astype(np.float64), b.astype(np.float64)
    t = [bd[r] * ad[c] for r in range(3) for c in range(3)]
    t += [(a[c] - b[c]).astype(np.float64) for c in range(3)]  # float subtraction, then widened (icp.cpp:314-344)
    return t, ad, bd


def check_exact(sums, terms, n, slack=None):
    """every sum within k * 2^-53 * sum|t| of the exact sum (plus the per-term rounding slack, p2l only)"""
    k = chain(n)
    for s, t in enumerate(terms):
        t = np.asarray(t, np.float64)
        exact = math.fsum(t.tolist())
        bound = k * U * float(np.sum(np.abs(t))) + (0.0 if slack is None else 2.0 * float(np.sum(slack[s])))
        assert abs(sums[s] - exact) <= bound, (n, s, sums[s], exact, bound)


@pytest.mark.parametrize("n", SIZES)
def test_reduce_against_exact_sum(ctx, oracle, n):
    """Catches: a block dropped or counted twice, a grid stride other than 256 B (a second-pass element skipped or
    added twice), a partial left over from an earlier, larger reduction, and `<=` instead of `<` at the acceptance
    (icp.cpp:553): max_dist is set to a distance that occurs, so at least one query sits exactly on it."""
    src, tgt = cloud(n, seed=n)
    if n >= 64:
        src[:, n // 3] = np.nan  # a NaN query: a non-finite distance, never accepted
    ctx.set_target(tgt)
    ctx.set_source(src)
    idx, dist = ctx.nn(binding.NN_EXACT)
    if n >= 64:
        assert not np.isfinite(dist[n // 3])
    fin = np.sort(dist[np.isfinite(dist)])
    for max_dist in (float(fin[len(fin) // 2]), 0.75):
        sums, cnt = ctx.reduce(max_dist)
        osums, ocnt = oracle.sums_canonical(src, tgt, idx, dist, max_dist)
        assert np.array_equal(sums.view(np.uint64), osums.view(np.uint64))
        acc = dist < np.float32(max_dist)
        assert cnt == ocnt == np.count_nonzero(acc)
        if max_dist != 0.75:
            assert np.count_nonzero(dist == np.float32(max_dist)) >= 1  # on the boundary: rejected
        t, ad, bd = nsum_terms(src, tgt, idx, acc)
        terms = t + [dist[acc].astype(np.float64)] + [ad[c] for c in range(3)] + [bd[c] for c in range(3)]
        check_exact(sums, terms, n)


@pytest.mark.parametrize("n", SIZES)
def test_reduce_p2l_against_exact_sum(ctx, oracle, n):
    """icpk_reduce_p2l, same tree, 28 sums.  Its terms are not exact in float64 (J = p x n and r = (p - q).n round),
    so the numpy terms carry a per-term bound: J_a has relative error u, r an absolute error <= 2u sum|(p - q)_c n_c|,
    J_a J_b then <= 4u |J_a J_b|, J_a r <= 5u |J_a| sum|(p - q)_c n_c|.  The kernel's and numpy's terms are both within
    it of the exact terms, hence the factor 2.  Zero normals (skipped pairs) are mixed in."""
    src, tgt = cloud(n, seed=7 + n)
    rng = np.random.default_rng(n)
    nrm = rng.normal(0, 1, tgt.shape)
    nrm = (nrm / np.linalg.norm(nrm, axis=0)).astype(np.float32)
    nrm[:, ::17] = 0
    ctx.set_target(tgt)
    ctx.set_target_normals(nrm)
    ctx.set_source(src)
    idx, dist = ctx.nn(binding.NN_EXACT)
    max_dist = float(np.sort(dist)[(3 * n) // 4])
    sums, cnt = ctx.reduce_p2l(max_dist)
    osums, ocnt = oracle.sums_p2l_canonical(src, tgt, nrm, idx, dist, max_dist)
    assert np.array_equal(sums.view(np.uint64), osums.view(np.uint64))
    acc = (dist < np.float32(max_dist)) & np.any(nrm[:, idx] != 0, axis=0)
    assert cnt == ocnt == np.count_nonzero(acc)
    p = src[:, acc].astype(np.float64)
    q = tgt[:, idx[acc]].astype(np.float64)
    m = nrm[:, idx[acc]].astype(np.float64)
    J = [p[1] * m[2] - p[2] * m[1], p[2] * m[0] - p[0] * m[2], p[0] * m[1] - p[1] * m[0], m[0], m[1], m[2]]
    r = ((p[0] - q[0]) * m[0] + (p[1] - q[1]) * m[1]) + (p[2] - q[2]) * m[2]
    R = np.abs((p[0] - q[0]) * m[0]) + np.abs((p[1] - q[1]) * m[1]) + np.abs((p[2] - q[2]) * m[2])
    terms, slack = [], []
    for a in range(6):
        for b in range(a, 6):
            terms.append(J[a] * J[b])
            slack.append(4 * U * np.abs(J[a] * J[b]))
    for a in range(6):
        terms.append(J[a] * r)
        slack.append(5 * U * np.abs(J[a]) * R)
    terms.append(dist[acc].astype(np.float64))
    slack.append(np.zeros(1))
    check_exact(sums, terms, n, slack)


def test_reduce_acceptance_edges(ctx, oracle):
    """Strict `<` with every distance exactly on max_dist (all rejected: `<=` would accept them), max_dist = 0 (count
    0, every sum +0.0: a stale partial of the reduction before would show), and a cloud where only the LAST query is
    accepted: it sits in the final, partial block of the second grid-stride pass (n = 65536 + 255), so a loop that
    stops after one pass, or a last block that is dropped, loses it."""
    n = 65536 + 255
    B, L = red_geometry(n)
    assert (B, L) == (256, 2) and (n - 1) - 256 * B < 256  # the last element: block 0 of the second pass ...
    assert (n - 1) % 256 == 254  # ... and not a full block's last lane
    rng = np.random.default_rng(3)
    tgt = (rng.uniform(-2, 2, (3, 2000)) + 5).astype(np.float32)
    src = (tgt[:, rng.integers(0, 2000, n)] + np.float32(30)).astype(np.float32)  # far from every target
    src[:, -1] = tgt[:, 11] + np.float32(1e-3)
    ctx.set_target(tgt)
    ctx.set_source(src)
    idx, dist = ctx.nn(binding.NN_EXACT)
    assert ctx.reduce(1e9)[1] == n  # a full reduction first: its partials must not leak into the ones below
    d_last = float(dist[-1])
    assert np.count_nonzero(dist <= np.float32(d_last)) == 1
    for max_dist, want in ((d_last, 0), (float(np.nextafter(np.float32(d_last), np.float32(1))), 1), (0.0, 0)):
        sums, cnt = ctx.reduce(max_dist)
        osums, ocnt = oracle.sums_canonical(src, tgt, idx, dist, max_dist)
        assert cnt == ocnt == want == np.count_nonzero(dist < np.float32(max_dist)), max_dist
        assert np.array_equal(sums.view(np.uint64), osums.view(np.uint64))
        if want == 0:
            assert not sums.view(np.uint64).any()  # +0.0 everywhere (not -0.0, not a leftover)
        else:
            t, ad, bd = nsum_terms(src, tgt, idx, dist < np.float32(max_dist))
            exact = [float(x[0]) for x in t] + [float(dist[-1])] + [float(ad[c, 0]) for c in range(3)] + \
                [float(bd[c, 0]) for c in range(3)]
            assert np.array_equal(sums, np.array(exact))  # one term: the tree adds only zeros to it
    # every distance ON the threshold: a lattice query set at exactly one target spacing from the targets
    tq = np.zeros((3, 1), np.float32) + np.float32(5)
    sq = np.repeat(tq + np.array([[0.5], [0], [0]], np.float32), 300, axis=1)
    ctx.set_target(tq)
    ctx.set_source(sq)
    idx, dist = ctx.nn(binding.NN_EXACT)
    assert np.all(dist == dist[0])
    sums, cnt = ctx.reduce(float(dist[0]))
    assert cnt == 0 and not sums.view(np.uint64).any()


# ---- the records path: the reduction inside icpk_align (device loop) and inside a lock-step group -------------------
LOOP_SIZES = [1_000_003, 131073, 65536 + 255, 65537, 65536, 65535, 257, 256, 1]  # large -> small


def loop_pairs():
    out = []
    for n in LOOP_SIZES:
        src, tgt = cloud(n, seed=31 + n, nt=4000)
        out.append((src, tgt))
    return out


def check_last_sweep(st, idx, dist, n, max_dist=0.75):
    """final_pairs / final_mse of the last sweep against its associations: count by numpy, mean by fsum"""
    acc = dist < np.float32(max_dist)
    cnt = int(np.count_nonzero(acc))
    assert st.final_pairs == cnt, (n, st.final_pairs, cnt)
    if cnt == 0:
        assert st.final_mse == 0.0
        return
    m = math.fsum(dist[acc].astype(np.float64).tolist()) / cnt
    rel = 2 * (chain(n) * U + 2.0 ** -24) + 2.0 ** -24  # tree, (float) of the mean, (float) of its square
    assert abs(float(np.float32(st.final_mse)) - m * m) <= 1.01 * rel * m * m, (n, st.final_mse, m * m)


def test_loop_reduction_single_path(ctx):
    """One fixed iteration through icpk_align (grid sweep, device loop: the 32-byte records path of
    assoc_reduce_body): final_pairs / final_mse agree with the exact statistics of the sweep they come from."""
    for (src, tgt), n in zip(loop_pairs(), LOOP_SIZES):
        ctx.set_target(tgt)
        ctx.set_source(src)
        T, st, rc = ctx.align(max_iterations=1, fixed_iterations=1)
        idx, dist = ctx.get_associations()
        if n < 3:  # fewer than min_pairs queries: the fallback of icp.cpp:163-182
            assert rc == st.status == binding.W_TOO_FEW_PAIRS, n
            continue
        assert rc == 0 and st.iterations == 1 and st.nn_launches == 2, n
        check_last_sweep(st, idx, dist, n)


def test_loop_reduction_lockstep_slot_reuse(monkeypatch):
    """The same pairs in lock step, 4 to a group, large -> small over 3 groups on the two alternating slot sets: the
    1-point pair of group 2 lands in the slot whose partial array held the 1 000 003-point pair's 256 blocks (stage 2
    must read only its own nblocks = 1, everything else as +0.0).  T, statistics and associations equal the single
    path's bit for bit, and the counts equal numpy's."""
    monkeypatch.setenv("ICPK_BATCH_GROUP", "4")
    pairs = loop_pairs()
    assert len(pairs) == 9 and LOOP_SIZES[0] == 1_000_003 and LOOP_SIZES[8] == 1  # pair 8: slot 0 of set 0, as pair 0
    assert red_geometry(LOOP_SIZES[0])[0] == 256 and red_geometry(LOOP_SIZES[8])[0] == 1
    kw = dict(max_iterations=1, fixed_iterations=1)
    for solve in (binding.SOLVE_REFERENCE, binding.SOLVE_KABSCH):
        with binding.Context(0) as single:
            want = []
            for s, t in pairs:
                single.set_target(t)
                single.set_source(s)
                T, st, rc = single.align(solve=solve, **kw)
                want.append((T.copy(), st, rc, *single.get_associations()))
        with binding.Context(0) as c:
            T, st, rc, assoc = c.align_batch(pairs, associations=True, solve=solve, **kw)
        assert rc == binding.W_TOO_FEW_PAIRS  # (the 1-point pair's fallback; every other pair: 0)
        for k, n in enumerate(LOOP_SIZES):
            idx, dist = assoc[k]
            assert st[k].status == (binding.W_TOO_FEW_PAIRS if n < 3 else 0), n
            if n >= 3:
                check_last_sweep(st[k], idx, dist, n)
            Tw, sw, rw, iw, dw = want[k]
            assert np.array_equal(T[k].view(np.uint32), Tw.view(np.uint32)), (solve, n)
            assert (st[k].iterations, st[k].status, st[k].final_pairs) == (sw.iterations, sw.status, sw.final_pairs)
            assert np.float32(st[k].final_mse).view(np.uint32) == np.float32(sw.final_mse).view(np.uint32), (solve, n)
            assert np.array_equal(idx, iw) and np.array_equal(dist.view(np.uint32), dw.view(np.uint32)), (solve, n)
