"""Soak test (tools only): the neighbourhood kernels (voxel grid, normals, outlier filters, pose scoring, FPFH and
matching, colour gradients) against the numpy models of their rules (tests/*_model.py), bit for bit, on random and
degenerate clouds with radii below every spacing, above the diameter and exactly on a lattice distance (cases:
tests/soak_cases.py).
usage: soak_neighbourhoods.py [n] [seed0] [feature ...]   (default: every feature, each from its own seed0 + 1000 * k)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from icp_slam_prototype_amd import binding
import soak_cases

n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 72
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 120000
features = sys.argv[3:] or list(soak_cases.FEATURES)
ctx = binding.Context(0)
total = total_bad = 0
for f in features:
    k = soak_cases.FEATURES.index(f)
    done, bad = soak_cases.soak_neighbourhoods(ctx, f, n_cases, seed0 + 1000 * k, log=lambda m: print(f, m, flush=True))
    print(f"{f}: {done} cases, {bad} mismatches", flush=True)
    total, total_bad = total + done, total_bad + bad
print("done:", total, "cases,", total_bad, "mismatches")
sys.exit(1 if total_bad else 0)
