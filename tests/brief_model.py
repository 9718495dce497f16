"""THE BRIEF RULE and THE MATCH RULE of include/icpk.h (K32) restated in numpy, int64 throughout.  The two committed
tables are read through the library (icpk_brief_pattern, icpk_brief_boundaries), so the model and the code under test
compare against the same bytes; everything else is written here on its own.  Shared by the host and the GPU tests."""
import functools

import numpy as np

from icp_slam_prototype_amd import binding

B, R2, OFF, BOX, NONE = 15, 225, 13, 2, 257


@functools.lru_cache(None)
def pattern():
    t = binding.brief_pattern()
    t.setflags(write=False)
    return t


@functools.lru_cache(None)
def boundaries():
    return [(int(x), int(y)) for x, y in binding.brief_boundaries()]


def gray(img):
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        return img.astype(np.int64)
    b, g, r = (img[..., k].astype(np.int64) for k in range(3))
    return (1868 * b + 9617 * g + 4899 * r + 8192) >> 14


def bin_of(m10, m01):
    """the orientation bin of one pair of integer moments (python integers: no overflow to think about)"""
    m10, m01 = int(m10), int(m01)
    if m10 == 0 and m01 == 0:
        return 0
    if m10 > 0 and m01 >= 0:
        q, x, y = 0, m10, m01
    elif m10 <= 0 and m01 > 0:
        q, x, y = 1, m01, -m10
    elif m10 < 0 and m01 <= 0:
        q, x, y = 2, -m10, -m01
    else:
        q, x, y = 3, -m01, m10
    c = sum(1 for bx, by in boundaries() if bx * y - by * x > 0)
    return (8 * q + c) % 32


def pixel_of(kp, rows, cols):
    """(x, y, described) per key point: nearest pixel (ties to even), described iff B <= x < cols - B, B <= y < rows - B"""
    kp = np.asarray(kp, np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        near = (np.abs(kp) < 1e6).all(1)  # (NaN, infinities and anything far outside any image describe nothing)
    r = np.rint(np.where(near[:, None], kp, -1).astype(np.float64)).astype(np.int64)
    ok = near & (r[:, 0] >= B) & (r[:, 0] < cols - B) & (r[:, 1] >= B) & (r[:, 1] < rows - B)
    return r[:, 0], r[:, 1], ok


def describe(img, kp, upright=False):
    """(words (n, 8) uint32, bin (n,) uint8, valid (n,) uint8)"""
    g = gray(img)
    rows, cols = g.shape
    x, y, ok = pixel_of(kp, rows, cols)
    n = len(x)
    words, bins = np.zeros((n, 8), np.uint32), np.zeros(n, np.uint8)
    if not ok.any():
        return words, bins, ok.astype(np.uint8)
    # S at every pixel whose box lies inside the image, by an integral image
    ii = np.zeros((rows + 1, cols + 1), np.int64)
    ii[1:, 1:] = g.cumsum(0).cumsum(1)
    w = 2 * BOX + 1
    S = np.zeros((rows, cols), np.int64)
    S[BOX:rows - BOX, BOX:cols - BOX] = ii[w:, w:] - ii[:-w, w:] - ii[w:, :-w] + ii[:-w, :-w]
    xs, ys = x[ok], y[ok]
    dy, dx = np.mgrid[-B:B + 1, -B:B + 1]
    disc = dx * dx + dy * dy <= R2
    dx, dy = dx[disc], dy[disc]
    win = g[ys[:, None] + dy[None, :], xs[:, None] + dx[None, :]]
    m10, m01 = (win * dx).sum(1), (win * dy).sum(1)
    b = np.zeros(len(xs), np.int64) if upright else np.array([bin_of(p, q) for p, q in zip(m10, m01)], np.int64)
    t = pattern()[b].astype(np.int64)  # (m, 256, 4)
    sa = S[ys[:, None] + t[:, :, 1], xs[:, None] + t[:, :, 0]]
    sb = S[ys[:, None] + t[:, :, 3], xs[:, None] + t[:, :, 2]]
    words[ok] = np.packbits(sa < sb, axis=1, bitorder="little").view("<u4")
    bins[ok] = b
    return words, bins, ok.astype(np.uint8)


def hamming(ws, wt):
    """(ns, nt) int64 Hamming distances"""
    a = np.unpackbits(np.ascontiguousarray(ws, "<u4").view(np.uint8).reshape(len(ws), 32), axis=1).astype(np.float32)
    b = np.unpackbits(np.ascontiguousarray(wt, "<u4").view(np.uint8).reshape(len(wt), 32), axis=1).astype(np.float32)
    return np.rint(a @ (1 - b).T + (1 - a) @ b.T).astype(np.int64)  # (exact: sums of at most 256 ones)


def match(ws, vs, wt, vt, max_hamming=48, ratio=None, mutual=True):
    """(src_kp, tgt_kp, H, H2) int32 of the kept pairs, source order"""
    ws, wt = np.asarray(ws, np.uint32).reshape(-1, 8), np.asarray(wt, np.uint32).reshape(-1, 8)
    vs, vt = np.asarray(vs).astype(bool), np.asarray(vt).astype(bool)
    empty = tuple(np.zeros(0, np.int32) for _ in range(4))
    if not vs.any() or not vt.any():
        return empty
    D = hamming(ws, wt)
    big = 1 << 20
    D = np.where(vs[:, None] & vt[None, :], D, big)
    j = D.argmin(1)  # (the first minimum: the lowest j)
    i_all = np.arange(len(ws))
    H = D[i_all, j]
    rest = D.copy()
    rest[i_all, j] = big
    H2 = rest.min(1) if len(wt) > 1 else np.full(len(ws), big)
    H2 = np.where(H2 >= big, NONE, H2)
    keep = vs & (H < big) & (H <= max_hamming)
    if ratio is not None and ratio[0] > 0:
        keep &= H * ratio[1] < H2 * ratio[0]
    if mutual:
        keep &= D.argmin(0)[j] == i_all
    k = np.nonzero(keep)[0]
    return k.astype(np.int32), j[k].astype(np.int32), H[k].astype(np.int32), H2[k].astype(np.int32)
