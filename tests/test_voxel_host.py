"""Voxel-grid downsampling (K11) without a GPU: the numpy model of the rule (tests/voxel_model.py) against a point-by-
point restatement and against the plain float64 mean, and the library's two entry points on a NULL context."""
import ctypes as C

import numpy as np
import pytest

import voxel_model as vm
from icp_slam_prototype_amd import binding, build, synth


def _small_clouds():
    rng = np.random.default_rng(11)
    out = []
    for n, leaf in ((1, 0.05), (7, 0.05), (300, 0.05), (2000, 0.2), (1500, 0.013)):
        p = rng.uniform(-1.5, 1.5, (3, n)).astype(np.float32)
        out.append((p, leaf))
    p = rng.uniform(-0.4, 0.4, (3, 800)).astype(np.float32)
    p[:, 100:200] = p[:, :100]                                     # duplicates
    p[:, 200:260] = np.float32(0.05) * rng.integers(-4, 5, (3, 60)).astype(np.float32)  # on voxel faces
    p[0, 260:270] = np.float32(-0.0)
    p[1, 270] = np.nan
    p[2, 271] = np.inf
    p[0, 272] = -np.inf
    p[0, 273] = np.float32(0.05) * np.float32(2 ** 20 + 3)         # beyond the limit: dropped
    p[1, 274] = -np.float32(0.05) * np.float32(2 ** 20 + 3)
    out.append((p, 0.05))
    out.append((np.zeros((3, 0), np.float32), 0.05))
    return out


@pytest.mark.parametrize("mode", [vm.FIRST, vm.CENTROID])
def test_model_equals_brute_force(mode):
    """Same groups, same order, same bits -- with and without normals."""
    rng = np.random.default_rng(5)
    for p, leaf in _small_clouds():
        a, b = vm.downsample(p, leaf, mode), vm.brute_force(p, leaf, mode)
        assert vm.same(a, b) is None, (p.shape, leaf, vm.same(a, b))
        nr = rng.normal(0, 1, p.shape)
        nr /= np.maximum(np.linalg.norm(nr, axis=0), 1e-9)
        nr = nr.astype(np.float32)
        nr[:, ::7] = 0.0  # pixels without a normal
        a, b = vm.downsample(p, leaf, mode, nr), vm.brute_force(p, leaf, mode, nr)
        assert vm.same(a, b) is None, (p.shape, leaf, vm.same(a, b))
        assert a["n_out"] + 0 == len(a["count"]) and a["count"].sum() + a["n_dropped"] == p.shape[1]
    # the special cloud really exercises what it is for
    p, leaf = _small_clouds()[-2]
    r = vm.downsample(p, leaf, mode)
    assert r["n_dropped"] == 5 and (r["count"] > 1).any() and (r["out_of_point"][[270, 271, 272, 273, 274]] == -1).all()
    # order: first_index ascends, and every point's output is the voxel of its first member
    assert (np.diff(r["first_index"]) > 0).all()
    assert np.array_equal(r["out_of_point"][r["first_index"]], np.arange(r["n_out"]))


def _ulp32(x):
    return np.spacing(np.abs(x.astype(np.float32))).astype(np.float64)


@pytest.mark.parametrize("leaf,n_out,max_members", [(0.02, 43299, 15), (0.05, 8206, 64), (0.2, 591, 820)])
def test_centroid_close_to_float64_mean(leaf, n_out, max_members):
    """|model - (float)mean| <= max(ulp32(model), ulp32(mean)) + leaf * 2^-30 per coordinate: the fixed point moves a
    coordinate by at most leaf * 2^-30 (each member's fraction is rounded to 2^-30 of a leaf, by at most half of that;
    the divisions and the final product add float64 roundings far below it), and rounding to float is monotonic, so
    two reals that close land on the same or on neighbouring floats.  Derived, not measured."""
    src = synth.kinect_pair()["source"]
    assert src.shape[1] == 91870
    r = vm.downsample(src, leaf, vm.CENTROID)
    assert (r["n_out"], int(r["count"].max())) == (n_out, max_members)
    sums = np.zeros((3, r["n_out"]), np.float64)
    for c in range(3):
        np.add.at(sums[c], r["out_of_point"], src[c].astype(np.float64))
    mean = (sums / r["count"].astype(np.float64)).astype(np.float32)
    model = r["points"]
    err = np.abs(model.astype(np.float64) - mean.astype(np.float64))
    bound = np.maximum(_ulp32(model), _ulp32(mean)) + float(np.float32(leaf)) * 2.0 ** -30
    print(f"leaf {leaf}: n_out {r['n_out']}, max members {r['count'].max()}, worst err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    # and the centroid lies in its voxel (closed on the upper side by the final roundings)
    _, v, _ = vm.voxel_coords(src, leaf)
    lo = v[:, r["first_index"]] * float(np.float32(leaf))
    assert (model >= (lo - _ulp32(model)).astype(np.float32)).all()
    assert (model <= (lo + float(np.float32(leaf)) + _ulp32(model))).all()


def test_float_and_double_quotients_disagree_somewhere():
    """The rule divides in float64: there are float32 coordinates whose voxel differs when p / leaf is taken in float32
    (about six in a million between 0.5 and 6 m at leaf 0.05).  The GPU test relies on such inputs existing."""
    p = np.random.default_rng(3).uniform(0.5, 6.0, 3_000_000).astype(np.float32)
    leaf = np.float32(0.05)
    v64 = np.floor(p.astype(np.float64) / np.float64(leaf))
    v32 = np.floor(p / leaf).astype(np.float64)
    share = np.count_nonzero(v64 != v32) / p.size
    assert 1e-6 < share < 3e-5, share


def test_null_context_is_rejected():
    """Both entry points exist and refuse a NULL context, as the others do (tests/test_abi.py)."""
    build.build()
    lib = binding.load()
    assert lib.icpk_voxel_downsample(None, 0, 0.05, binding.VOXEL_CENTROID, None, None) == binding.E_ARG
    n = C.c_int32(7)
    assert lib.icpk_get_voxel_groups(None, C.byref(n), None, None, None, None) == binding.E_ARG
    assert n.value == 7
    assert (binding.VOXEL_FIRST, binding.VOXEL_CENTROID) == (0, 1)
    assert {"icpk_voxel_downsample", "icpk_get_voxel_groups"} <= set(binding.SYMBOLS)
