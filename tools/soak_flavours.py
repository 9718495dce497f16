"""Soak test (tools only): whole alignments of the newer flavours (point-to-plane, robust Kabsch / point-to-plane,
plane-to-plane, colored), grid scan + device loop vs exact kernel + host loop on one context, bit for bit (transform,
status, pair count, mse, associations, moved source, trace, robust trace; cases: tests/soak_cases.py).
usage: soak_flavours.py [n] [seed0] [flavour ...]   (default: every flavour, each from its own seed0 + 1000 * k)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from icp_slam_prototype_amd import binding
import soak_cases

n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 200
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 130000
flavours = sys.argv[3:] or list(soak_cases.FLAVOURS)
ctx = binding.Context(0)
total = total_bad = 0
for f in flavours:
    k = soak_cases.FLAVOURS.index(f)
    done, bad, tally = soak_cases.soak_flavours(ctx, f, n_cases, seed0 + 1000 * k, log=lambda m: print(f, m, flush=True))
    print(f"{f}: {done} cases, {bad} mismatches, {tally}", flush=True)
    total, total_bad = total + done, total_bad + bad
print("done:", total, "cases,", total_bad, "mismatches")
sys.exit(1 if total_bad else 0)
