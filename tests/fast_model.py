"""Plain restatement of the FAST contract of include/icpk.h (OpenCV 3.2's cv::cvtColor(CV_BGR2GRAY) and scalar
FAST_t<patternSize>, features2d/src/fast.cpp) -- TEST INFRASTRUCTURE, never used by the product.

`detect_loop` is written as FAST_t's loops (three score rows, suppression of the previous row while the current one is
scored); `detect` is the same contract vectorised over the image, for frame-sized inputs.  Both return
(kp_xy (n, 2) float32, response (n,) float32) in FAST_t's push order (row-major).

Golden fixtures from a real OpenCV run can be added as files under tests/golden/ and compared against `detect` by one
test file; none exist yet (parity with OpenCV itself is unpinned)."""
import numpy as np

TYPE_5_8, TYPE_7_12, TYPE_9_16 = 0, 1, 2

# OpenCV makeOffsets order, (dx, dy)
CIRCLE = {
    16: [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1),
         (-3, 0), (-3, 1), (-2, 2), (-1, 3)],
    12: [(0, 2), (1, 2), (2, 1), (2, 0), (2, -1), (1, -2), (0, -2), (-1, -2), (-2, -1), (-2, 0), (-2, 1), (-1, 2)],
}
QUICK = [[(0, 8)], [(2, 10), (4, 12), (6, 14)], [(1, 9), (3, 11), (5, 13), (7, 15)]]  # stop after a group leaves d == 0


def pattern_of(type_):
    if type_ == TYPE_9_16:
        return 16
    if type_ == TYPE_7_12:
        return 12
    raise ValueError("FAST type out of scope")


def wrapped(P):
    """the offset table extended to 25 entries: pixel[k] = pixel[k - P]"""
    return [CIRCLE[P][k % P] for k in range(25)]


def bgr_to_gray(bgr):
    bgr = np.asarray(bgr, np.uint8).astype(np.int64)
    b, g, r = bgr[..., 0], bgr[..., 1], bgr[..., 2]
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def as_gray(img):
    img = np.asarray(img, np.uint8)
    return bgr_to_gray(img) if img.ndim == 3 else img


def _cls(x, v, t):
    return 1 if x < v - t else (2 if x > v + t else 0)


def corner_score(circle, v, P):
    """cornerScore<P> in closed form: M - 1 over the P arcs of P/2 + 1 circle pixels"""
    K = P // 2
    d = [v - int(x) for x in circle]
    M = None
    for s in range(P):
        arc = [d[(s + j) % P] for j in range(K + 1)]
        m = max(min(arc), -max(arc))
        M = m if M is None else max(M, m)
    return M - 1


def pixel_test(img, y, x, t, P):
    """FAST_t's test of one candidate pixel: (is_corner, score)"""
    K = P // 2
    tab = wrapped(P)
    v = int(img[y, x])
    c = [int(img[y + dy, x + dx]) for dx, dy in tab]
    d = None
    for group in QUICK:
        for a, b in group:
            e = _cls(c[a], v, t) | _cls(c[b], v, t)
            d = e if d is None else d & e
        if d == 0:
            return False, 0
    for bit, darker in ((1, True), (2, False)):
        if not d & bit:
            continue
        count = 0
        for k in range(P + K + 1):
            hit = c[k] < v - t if darker else c[k] > v + t
            if hit:
                count += 1
                if count > K:
                    return True, corner_score(c[:P], v, P)
            else:
                count = 0
    return False, 0


def detect_loop(img, threshold=60, nonmax=True, type_=TYPE_7_12):
    P = pattern_of(type_)
    g = as_gray(img)
    rows, cols = g.shape
    t = min(max(int(threshold), 0), 255)
    kp, resp = [], []
    if rows < 7 or cols < 7:
        return np.zeros((0, 2), np.float32), np.zeros(0, np.float32)
    buf = [np.zeros(cols, np.int64) for _ in range(3)]
    cpos = [[] for _ in range(3)]
    for i in range(3, rows - 2):
        curr = buf[(i - 3) % 3]
        curr[:] = 0
        corners = cpos[(i - 3) % 3]
        corners.clear()
        if i < rows - 3:
            for j in range(3, cols - 3):
                ok, s = pixel_test(g, i, j, t, P)
                if ok:
                    corners.append(j)
                    if nonmax:
                        curr[j] = s
        if i == 3:
            continue
        prev, pprev = buf[(i - 4 + 3) % 3], buf[(i - 5 + 3) % 3]
        for j in cpos[(i - 4 + 3) % 3]:
            s = prev[j]
            if not nonmax or (s > prev[j + 1] and s > prev[j - 1] and s > pprev[j - 1] and s > pprev[j] and
                              s > pprev[j + 1] and s > curr[j - 1] and s > curr[j] and s > curr[j + 1]):
                kp.append((j, i - 1))
                resp.append(s)
    return np.array(kp, np.float32).reshape(-1, 2), np.array(resp, np.float32)


def _runs(mask, P):
    """mask (..., P) bool -> does a circular run of P/2 + 1 set entries exist"""
    K = P // 2
    e = np.concatenate([mask, mask], axis=-1)
    r = e[..., :P].copy()
    for i in range(1, K + 1):
        r &= e[..., i:i + P]
    return r.any(axis=-1)


def score_map(img, threshold=60, type_=TYPE_7_12):
    """(corner (rows, cols) bool, score (rows, cols) int64) of every pixel, vectorised"""
    P = pattern_of(type_)
    K = P // 2
    g = as_gray(img).astype(np.int64)
    rows, cols = g.shape
    t = min(max(int(threshold), 0), 255)
    corner = np.zeros((rows, cols), bool)
    score = np.zeros((rows, cols), np.int64)
    if rows < 7 or cols < 7:
        return corner, score
    v = g[3:rows - 3, 3:cols - 3]
    c = np.stack([g[3 + dy:rows - 3 + dy, 3 + dx:cols - 3 + dx] for dx, dy in wrapped(P)[:16]], axis=-1)
    cls = np.where(c < (v - t)[..., None], 1, np.where(c > (v + t)[..., None], 2, 0))
    alive = np.ones(v.shape, bool)
    d = None
    for group in QUICK:
        for a, b in group:
            e = cls[..., a] | cls[..., b]
            d = e if d is None else d & e
        alive &= d != 0
    c = c[..., :P]
    dark = _runs(c < (v - t)[..., None], P) & ((d & 1) != 0)
    bright = _runs(c > (v + t)[..., None], P) & ((d & 2) != 0)
    cn = alive & (dark | bright)
    dd = v[..., None] - c
    M = None
    for s in range(P):
        arc = np.stack([dd[..., (s + j) % P] for j in range(K + 1)], axis=-1)
        m = np.maximum(arc.min(-1), -arc.max(-1))
        M = m if M is None else np.maximum(M, m)
    corner[3:rows - 3, 3:cols - 3] = cn
    score[3:rows - 3, 3:cols - 3] = np.where(cn, M - 1, 0)
    return corner, score


def detect(img, threshold=60, nonmax=True, type_=TYPE_7_12):
    corner, score = score_map(img, threshold, type_)
    rows, cols = corner.shape
    keep = corner.copy()
    if nonmax:
        pad = np.zeros((rows + 2, cols + 2), np.int64)
        pad[1:-1, 1:-1] = score
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dy or dx:
                    keep &= score > pad[1 + dy:1 + dy + rows, 1 + dx:1 + dx + cols]
    y, x = np.nonzero(keep)  # row-major
    resp = score[y, x].astype(np.float32) if nonmax else np.zeros(len(y), np.float32)
    return np.stack([x, y], 1).astype(np.float32).reshape(-1, 2), resp


def _circle_image(P, positions, v=100, hi=200, size=15):
    """a neutral image whose centre pixel has the circle `positions` (indices of the P-table) set to `hi`"""
    img = np.full((size, size), v, np.uint8)
    c = size // 2
    for k in positions:
        dx, dy = CIRCLE[P][k % P]
        img[c + dy, c + dx] = hi
    return img, (c, c)


def hand_cases():
    """(name, image, kwargs, check) with known answers; check(kp, resp) -> bool.  Shared by the host and device tests."""
    out = []

    def has(kp, xy):
        return any((kp[:, 0] == xy[0]) & (kp[:, 1] == xy[1])) if len(kp) else False

    img = np.zeros((11, 11), np.uint8)
    img[5, 5] = 255
    for ty in (TYPE_7_12, TYPE_9_16):
        out.append((f"single_bright_pixel_{ty}", img, dict(threshold=60, type_=ty),
                    lambda kp, r: kp.tolist() == [[5, 5]] and r.tolist() == [254]))
    sq = np.zeros((20, 20), np.uint8)
    sq[8:, 8:] = 200
    # (with suppression the flat square's corner ties with its diagonal neighbour's: both go)
    out.append(("bright_square_corner", sq, dict(threshold=60, nonmax=False, type_=TYPE_9_16),
                lambda kp, r: has(kp, (8, 8)) and all(abs(x - 8) <= 2 and abs(y - 8) <= 2 for x, y in kp)))
    edge = np.zeros((16, 16), np.uint8)
    edge[:, 8:] = 200
    out.append(("straight_edge_9_16", edge, dict(threshold=60, type_=TYPE_9_16), lambda kp, r: len(kp) == 0))
    for surround, want in ((160, False), (161, True)):
        im = np.full((11, 11), surround, np.uint8)
        im[5, 5] = 100
        out.append((f"threshold_equality_{surround}", im, dict(threshold=60, type_=TYPE_9_16),
                    (lambda kp, r: kp.tolist() == [[5, 5]] and r.tolist() == [60]) if want else
                    (lambda kp, r: len(kp) == 0)))
    wrap, c = _circle_image(16, [13, 14, 15, 0, 1, 2, 3, 4, 5])
    out.append(("arc_wrapping_past_0", wrap, dict(threshold=60, nonmax=False, type_=TYPE_9_16),
                lambda kp, r, c=c: has(kp, c)))
    short, c = _circle_image(16, [13, 14, 15, 0, 1, 2, 3, 4])
    out.append(("arc_of_8_is_no_corner", short, dict(threshold=60, nonmax=False, type_=TYPE_9_16),
                lambda kp, r, c=c: not has(kp, c)))
    q17, c = _circle_image(12, [1, 2, 3, 4, 5, 6, 7])
    out.append(("quick_test_rejects_7_12_arc_1_to_7", q17, dict(threshold=60, nonmax=False, type_=TYPE_7_12),
                lambda kp, r, c=c: not has(kp, c)))
    q06, c = _circle_image(12, [0, 1, 2, 3, 4, 5, 6])
    out.append(("7_12_arc_0_to_6_is_a_corner", q06, dict(threshold=60, nonmax=False, type_=TYPE_7_12),
                lambda kp, r, c=c: has(kp, c)))
    two = np.zeros((12, 13), np.uint8)
    two[6, 6] = two[6, 7] = 255
    out.append(("equal_neighbours_suppress_each_other", two, dict(threshold=60, type_=TYPE_9_16),
                lambda kp, r: len(kp) == 0))
    out.append(("equal_neighbours_without_suppression", two, dict(threshold=60, nonmax=False, type_=TYPE_9_16),
                lambda kp, r: kp.tolist() == [[6, 6], [7, 6]] and r.tolist() == [0, 0]))
    bord = np.zeros((12, 12), np.uint8)
    bord[2, 5] = bord[5, 2] = bord[8, 5] = bord[5, 8] = 255  # y = 2, x = 2, y = rows - 4, x = cols - 4
    out.append(("border_pixels_never_reported", bord, dict(threshold=60, type_=TYPE_9_16),
                lambda kp, r: kp.tolist() == [[8, 5], [5, 8]]))  # (row-major)
    out.append(("t0_single_bright_pixel", img, dict(threshold=0, type_=TYPE_9_16),
                lambda kp, r: kp.tolist() == [[5, 5]] and r.tolist() == [254]))
    rnd = np.random.default_rng(5).integers(0, 256, (24, 40)).astype(np.uint8)
    for ty in (TYPE_7_12, TYPE_9_16):
        out.append((f"t255_nothing_{ty}", rnd, dict(threshold=255, nonmax=False, type_=ty), lambda kp, r: len(kp) == 0))
        out.append((f"t0_inside_candidates_{ty}", rnd, dict(threshold=0, nonmax=False, type_=ty),
                    lambda kp, r: len(kp) > 0 and kp[:, 0].min() >= 3 and kp[:, 1].min() >= 3 and
                    kp[:, 0].max() <= 36 and kp[:, 1].max() <= 20))
    six = np.zeros((6, 6), np.uint8)
    six[3, 3] = 255
    out.append(("6x6_has_no_candidates", six, dict(threshold=0, nonmax=False, type_=TYPE_9_16), lambda kp, r: len(kp) == 0))
    seven = np.zeros((7, 7), np.uint8)
    seven[3, 3] = 255
    for ty in (TYPE_7_12, TYPE_9_16):
        out.append((f"7x7_one_candidate_{ty}", seven, dict(threshold=60, type_=ty),
                    lambda kp, r: kp.tolist() == [[3, 3]] and r.tolist() == [254]))
    return out
