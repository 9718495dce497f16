#!/usr/bin/env python3
"""Writes icp_slam_prototype_amd/csrc/brief_table.h: the two committed tables of THE BRIEF RULE (include/icpk.h, K32).

Run once; the committed header is the rule, this tool is only how it was made.  Nothing at build or test time runs it.

  BRIEF_BOUNDARY  the 8 bin boundaries of the first quadrant as integer directions: (round(2^30 cos b), round(2^30 sin b))
                  for b = (j + 1/2) 11.25 degrees, j = 0 .. 7.
  BRIEF_TABLE     32 bins x 256 tests x (ax, ay, bx, by), int8.  Bin 0: offsets drawn uniformly from the integer offsets
                  with x^2 + y^2 <= 169 (listed row-major, y outer, both ascending) with icpk_set_subsample's finaliser,
                  z = SEED + (t + 1) 0x9E3779B97F4A7C15 + d 0xD1B54A32D192ED03, index = (uint32)(mix(z) >> 32) mod count:
                  a from draw d = 0, b from the first later draw whose offset differs from a in every bin.  Bin k: the
                  offset rotated by k 11.25 degrees and moved to the nearest integer offset inside the same disc (of the
                  four lattice points around it; multiples of 90 degrees are exact).
"""
import math
import os

SEED = 0x4252494546  # "BRIEF"
BINS, TESTS, R2 = 32, 256, 169
M64 = (1 << 64) - 1


def mix(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(t, d, count):
    return (mix(SEED + (t + 1) * 0x9E3779B97F4A7C15 + d * 0xD1B54A32D192ED03) >> 32) % count


def rotate(p, k):
    x, y = p
    for _ in range(k // 8):  # quarter turns, exact
        x, y = -y, x
    k %= 8
    if k == 0:
        return (x, y)
    a = math.radians(k * 11.25)
    rx, ry = x * math.cos(a) - y * math.sin(a), x * math.sin(a) + y * math.cos(a)
    best = None
    for cx in (math.floor(rx), math.floor(rx) + 1):
        for cy in (math.floor(ry), math.floor(ry) + 1):
            if cx * cx + cy * cy > R2:
                continue
            d = (cx - rx) ** 2 + (cy - ry) ** 2
            if best is None or d < best[0]:
                best = (d, cx, cy)
    return (best[1], best[2])


def main():
    offsets = [(x, y) for y in range(-13, 14) for x in range(-13, 14) if x * x + y * y <= R2]
    rot = {p: [rotate(p, k) for k in range(BINS)] for p in offsets}
    table = [[None] * TESTS for _ in range(BINS)]
    for t in range(TESTS):
        a = offsets[draw(t, 0, len(offsets))]
        d = 1
        while True:
            b = offsets[draw(t, d, len(offsets))]
            if all(rot[a][k] != rot[b][k] for k in range(BINS)):
                break
            d += 1
        for k in range(BINS):
            table[k][t] = rot[a][k] + rot[b][k]
    bounds = [(round(2 ** 30 * math.cos(math.radians((j + 0.5) * 11.25))), round(2 ** 30 * math.sin(math.radians((j + 0.5) * 11.25))))
              for j in range(8)]
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "icp_slam_prototype_amd", "csrc", "brief_table.h")
    with open(out, "w") as f:
        f.write("// brief_table.h -- K32: the two tables of THE BRIEF RULE (include/icpk.h), made once by tools/make_brief_table.py.\n"
                "// The tables are the rule, the tool is not.  BRIEF_BOUNDARY: the bin boundaries (j + 1/2) 11.25 degrees, j = 0 .. 7,\n"
                "// as integer directions (x, y) of length 2^30.  BRIEF_TABLE: per bin and test the offsets (ax, ay, bx, by); bin 0 is\n"
                "// the drawn pattern, bin k the pattern turned by k 11.25 degrees; every offset has x^2 + y^2 <= 169.\n"
                "#pragma once\n#include <cstdint>\n\nnamespace icpk {\n\n")
        f.write("constexpr int32_t BRIEF_BOUNDARY[8][2] = {\n")
        for bx, by in bounds:
            f.write(f"    {{{bx}, {by}}},\n")
        f.write("};\n\n")
        f.write(f"constexpr int8_t BRIEF_TABLE[{BINS}][{TESTS}][4] = {{\n")
        for k in range(BINS):
            f.write(f"    /* bin {k:2d} */ {{\n")
            for t0 in range(0, TESTS, 8):
                f.write("        " + " ".join("{%d,%d,%d,%d}," % table[k][t] for t in range(t0, t0 + 8)) + "\n")
            f.write("    },\n")
        f.write("};\n\n}  // namespace icpk\n")


if __name__ == "__main__":
    main()
