"""K32 on the CPU: the committed tables, the bin, and the two host-only functions of THE BRIEF RULE and THE MATCH RULE
(include/icpk.h) against the numpy model of tests/brief_model.py, and what the descriptors do on the textured room.

Measured on the three pose pairs at 240 x 320 (first frame against second, mutual, H <= 48; kept / true, true meaning
both world points within 5 cm):
    yaw 24 deg, 0.22 m      oriented 789 / 558 (71 %)    upright  994 / 870
    yaw 48 deg, 0.41 m      oriented 600 / 299 (50 %)    upright  650 / 470
    yaw 5 deg, roll 30 deg  oriented 1179 / 1055 (89 %)  upright  358 / 4"""
import numpy as np
import pytest

import brief_cases as bc
import brief_model as bm
from icp_slam_prototype_amd import binding, build


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build()
    return binding.load()


def test_table_properties():
    t = bm.pattern().astype(np.int64)
    assert t.shape == (32, 256, 4)
    a, b = t[..., :2], t[..., 2:]
    assert ((a ** 2).sum(-1) <= 169).all() and ((b ** 2).sum(-1) <= 169).all()
    assert (a != b).any(-1).all()
    # bin 0 is the drawn pattern itself: bins 8, 16 and 24 are its exact quarter turns, (x, y) -> (-y, x)
    for k in (8, 16, 24):
        prev = t[k - 8]
        assert np.array_equal(t[k], np.stack([-prev[:, 1], prev[:, 0], -prev[:, 3], prev[:, 2]], 1))
    # every other bin is bin 0 turned by k 11.25 degrees, each offset within a lattice cell of the real one
    for k in range(32):
        ang = np.deg2rad(k * 11.25)
        for o in (0, 2):
            x, y = t[0][:, o], t[0][:, o + 1]
            rx, ry = x * np.cos(ang) - y * np.sin(ang), x * np.sin(ang) + y * np.cos(ang)
            assert (np.abs(t[k][:, o] - rx) < 1 + 1e-9).all() and (np.abs(t[k][:, o + 1] - ry) < 1 + 1e-9).all()
    # 256 different tests, offsets all over the disc
    assert len({tuple(r) for r in t[0]}) == 256
    assert len({tuple(r) for r in t[0][:, :2]} | {tuple(r) for r in t[0][:, 2:]}) > 250
    bd = np.array(bm.boundaries(), np.float64)
    assert np.allclose(np.degrees(np.arctan2(bd[:, 1], bd[:, 0])), (np.arange(8) + 0.5) * 11.25, atol=1e-7)
    assert np.allclose(np.hypot(bd[:, 0], bd[:, 1]), 2.0 ** 30, rtol=1e-8)


def test_bin_against_atan2_on_random_moments():
    rng = np.random.default_rng(5)
    m = np.concatenate([rng.integers(-(1 << 22), 1 << 22, (6000, 2)), rng.integers(-40, 41, (3000, 2))])
    checked = 0
    for m10, m01 in m:
        if m10 == 0 and m01 == 0:
            continue
        a = np.arctan2(float(m01), float(m10)) / np.deg2rad(11.25)
        if abs((a - 0.5) - np.rint(a - 0.5)) * np.deg2rad(11.25) < 1e-6:  # (closer than 1e-6 rad to a boundary)
            continue
        want = int(np.rint(a)) % 32
        assert binding.brief_bin(m10, m01) == want == bm.bin_of(m10, m01), (m10, m01)
        checked += 1
    assert checked > 8900


def test_bin_on_the_boundaries_in_all_four_quadrants_and_at_zero():
    assert binding.brief_bin(0, 0) == 0 == bm.bin_of(0, 0)
    for j, (bx, by) in enumerate(bm.boundaries()):
        x, y = bx, by
        for q in range(4):  # the boundary direction itself, turned by q quarter turns: the lower bin
            assert binding.brief_bin(x, y) == 8 * q + j == bm.bin_of(x, y), (j, q)
            # one unit to either side of it, across the direction
            nx, ny = (-1 if y > 0 else 1 if y < 0 else 0), (1 if x > 0 else -1 if x < 0 else 0)  # counter-clockwise of it
            assert binding.brief_bin(x + nx, y + ny) == (8 * q + j + 1) % 32 == bm.bin_of(x + nx, y + ny)
            assert binding.brief_bin(x - nx, y - ny) == 8 * q + j == bm.bin_of(x - nx, y - ny)
            x, y = -y, x
    # the axes are the centres of bins 0, 8, 16, 24; the diagonals of 4, 12, 20, 28
    for (x, y), k in {(7, 0): 0, (0, 7): 8, (-7, 0): 16, (0, -7): 24, (3, 3): 4, (-3, 3): 12, (-3, -3): 20, (3, -3): 28}.items():
        assert binding.brief_bin(x, y) == k == bm.bin_of(x, y)
    for m10, m01 in ((-2 ** 31, -2 ** 31), (2 ** 31 - 1, -2 ** 31), (-2 ** 31, 2 ** 31 - 1), (-2 ** 31, 0), (0, -2 ** 31)):
        assert binding.brief_bin(m10, m01) == bm.bin_of(m10, m01)  # (the ends of int32: nothing overflows)


@pytest.mark.parametrize("shape", bc.IMAGE_SHAPES)
@pytest.mark.parametrize("channels", (1, 3))
def test_describe_host_gives_the_models_bytes(shape, channels):
    img = bc.random_image(*shape, channels)
    for n in bc.KEYPOINT_COUNTS:
        kp = bc.border_keypoints(*shape, n)
        for upright in (False, True):
            w, b, v = binding.brief_describe_host(img, kp, upright)
            mw, mb, mv = bm.describe(img, kp, upright)
            assert w.tobytes() == mw.tobytes() and b.tobytes() == mb.tobytes() and v.tobytes() == mv.tobytes()
            assert (w[v == 0] == 0).all() and (b[v == 0] == 0).all()
            if upright:
                assert (b == 0).all()
    # every pixel of a small image: exactly the pixels B <= x < cols - B, B <= y < rows - B are described
    y, x = np.mgrid[-1:shape[0] + 1, -1:shape[1] + 1]
    kp = np.stack([x.ravel(), y.ravel()], 1).astype(np.float32)
    if len(kp) <= 20000:
        w, b, v = binding.brief_describe_host(img, kp)
        mw, mb, mv = bm.describe(img, kp)
        assert w.tobytes() == mw.tobytes() and b.tobytes() == mb.tobytes() and v.tobytes() == mv.tobytes()
        assert int(v.sum()) == max(shape[0] - 30, 0) * max(shape[1] - 30, 0)


def test_describe_host_edges():
    img = np.full((40, 40), 93, np.uint8)  # constant: m = 0, bin 0, no bit set (S is never less than itself)
    kp = np.float32([[20, 20], [15.5, 16.5], [14.5, 20], [np.nan, 20], [20, np.inf], [-1e30, 3], [24.49, 24.5]])
    w, b, v = binding.brief_describe_host(img, kp)
    assert list(v) == [1, 1, 0, 0, 0, 0, 1] and (b == 0).all() and (w == 0).all()  # (15.5 -> 16, 14.5 -> 14: ties to even)
    assert bm.describe(img, kp)[2].tolist() == list(v)
    w0, b0, v0 = binding.brief_describe_host(img, np.zeros((0, 2), np.float32))
    assert len(w0) == len(b0) == len(v0) == 0
    # the bins that occur on random content cover the circle, and the moments' sign convention is x right, y down
    ramp = np.tile(np.arange(64, dtype=np.uint8) * 3, (64, 1))
    assert binding.brief_describe_host(ramp, [[32, 32]])[1][0] == 0          # brighter to the right: 0 degrees
    assert binding.brief_describe_host(ramp.T.copy(), [[32, 32]])[1][0] == 8  # brighter downwards: 90 degrees
    assert binding.brief_describe_host(ramp[:, ::-1].copy(), [[32, 32]])[1][0] == 16
    rnd = bc.random_image(120, 160, 1)
    kp = bc.border_keypoints(120, 160, 600, seed=3)
    assert len(set(binding.brief_describe_host(rnd, kp)[1].tolist())) == 32


@pytest.mark.parametrize("sizes", bc.MATCH_SIZES)
def test_match_host_gives_the_models_bytes(sizes):
    ns, nt = sizes
    ws, vs = bc.descriptor_set(ns, 10 + ns)
    wt, vt = bc.descriptor_set(nt, 20 + nt)
    if ns and nt:
        wt[: min(ns, nt) // 2] = ws[: min(ns, nt) // 2] ^ np.uint32(1)  # near copies: small distances exist
    for mutual in (False, True):
        for ratio in (None, (8, 10), (1, 1)):
            for mh in (0, 48, 256):
                got = binding.brief_match_host(ws, vs, wt, vt, max_hamming=mh, ratio=ratio, mutual=mutual)
                want = bm.match(ws, vs, wt, vt, max_hamming=mh, ratio=ratio, mutual=mutual)
                for g, w in zip(got, want):
                    assert g.tobytes() == w.tobytes(), (sizes, mutual, ratio, mh)
    none = np.zeros_like(vt)
    assert len(binding.brief_match_host(ws, vs, wt, none, max_hamming=256, mutual=False)[0]) == 0
    assert len(binding.brief_match_host(ws, np.zeros_like(vs), wt, vt, max_hamming=256, mutual=False)[0]) == 0


def test_match_host_duplicates_and_a_single_target():
    ws, vs = bc.descriptor_set(40, 3, invalid=0.0)
    wt = np.concatenate([ws[:10], ws[:10], ws[10:20]])  # targets 0 .. 9 again at 10 .. 19
    vt = np.ones(len(wt), np.uint8)
    i, j, H, H2 = binding.brief_match_host(ws, vs, wt, vt, max_hamming=0, mutual=False)
    assert i.tolist() == list(range(20)) and j.tolist() == list(range(10)) + list(range(20, 30))  # the lowest j wins
    assert (H == 0).all() and (H2[:10] == 0).all() and (H2[10:] > 0).all()
    for ratio in ((8, 10), (1, 1), (65536, 1)):  # H == H2 fails any ratio
        i2 = binding.brief_match_host(ws, vs, wt, vt, max_hamming=0, ratio=ratio, mutual=False)[0]
        assert i2.tolist() == list(range(10, 20))
    one = binding.brief_match_host(ws[:3], vs[:3], wt[:1], vt[:1], max_hamming=256, mutual=False)
    assert one[3].tolist() == [257, 257, 257] and one[1].tolist() == [0, 0, 0]  # no other target: H2 = 257
    assert binding.brief_match_host(ws[:3], vs[:3], wt[:1], vt[:1], max_hamming=256, mutual=True)[0].tolist() == [0]


def test_host_functions_refuse_bad_arguments():
    img = np.zeros((40, 40), np.uint8)
    kp = np.float32([[20, 20]])
    lib = binding.load()
    import ctypes as C
    u8, fp = C.POINTER(C.c_uint8), C.POINTER(C.c_float)
    d = lambda image, rows, cols, ch, k, n, flags: lib.icpk_brief_describe_host(image, rows, cols, ch, k, n, flags, None, None, None)
    ip, kp_p = img.ctypes.data_as(u8), kp.ctypes.data_as(fp)
    assert d(ip, 40, 40, 1, kp_p, 1, 0) == binding.OK  # (every output may be NULL)
    for bad in ((None, 40, 40, 1, kp_p, 1, 0), (ip, 0, 40, 1, kp_p, 1, 0), (ip, 40, -1, 1, kp_p, 1, 0), (ip, 40, 40, 2, kp_p, 1, 0),
                (ip, 40, 40, 1, None, 1, 0), (ip, 40, 40, 1, kp_p, -1, 0), (ip, 40, 40, 1, kp_p, 1, 2),
                (ip, 40, 40, 1, kp_p, binding.BRIEF_MAX_KEYPOINTS + 1, 0)):
        assert d(*bad) == binding.E_ARG, bad
    ws, vs = bc.descriptor_set(4, 1)
    for kw in (dict(max_hamming=-1), dict(max_hamming=257), dict(ratio=(-1, 1)), dict(ratio=(1, 0)), dict(ratio=(65537, 1))):
        with pytest.raises(binding.IcpkError):
            binding.brief_match_host(ws, vs, ws, vs, **kw)
    p = binding.brief_match_params(to_clouds=True)  # (no clouds on the host)
    with pytest.raises(binding.IcpkError):
        binding.brief_match_host(ws, vs, ws, vs, params=p)


@pytest.mark.parametrize("name", [p[0] for p in bc.POSES])
def test_textured_room_true_share(name):
    """the model on the CPU, first frame against second: at least 30 % of the kept pairs are true at every pose"""
    r = bc.model_pair(name)
    kept, true = len(r["matches"][0]), int(r["true"].sum())
    print(f"{name}: oriented kept {kept}, true {true} ({100.0 * true / max(kept, 1):.0f} %)")
    assert kept >= 100 and true >= 0.30 * kept
    # the host functions agree with the model on real frames too
    bgr, _ = bc.frame(name)
    w, b, v = binding.brief_describe_host(bgr, r["tgt"][0])
    assert w.tobytes() == r["tgt"][1].tobytes() and b.tobytes() == r["tgt"][2].tobytes() and v.tobytes() == r["tgt"][3].tobytes()
    got = binding.brief_match_host(r["src"][1], r["src"][3], r["tgt"][1], r["tgt"][3], max_hamming=bc.MAX_HAMMING, mutual=True)
    assert all(g.tobytes() == m.tobytes() for g, m in zip(got, r["matches"]))


def test_textured_room_roll_needs_the_orientation():
    o, u = bc.model_pair("roll30"), bc.model_pair("roll30", upright=True)
    print(f"roll30: oriented true {int(o['true'].sum())}, upright kept {len(u['matches'][0])} true {int(u['true'].sum())}")
    assert u["true"].sum() < 0.1 * o["true"].sum()
