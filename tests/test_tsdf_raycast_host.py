"""The ray rule of the TSDF volume (K20) without a GPU: icpk_tsdf_raycast_pixels -- the host half of csrc/tsdf_rule.h,
the header the kernel includes -- against tests/tsdf_raycast_model.py bit for bit on every case of the table; the
table's counts; the accuracy of the ray cast on the analytic room; and the refusals."""
import ctypes as C

import numpy as np
import pytest

import tsdf_cases as tc
import tsdf_raycast_cases as rc
import tsdf_raycast_model as rm
from icp_slam_prototype_amd import binding, build


@pytest.fixture(scope="module")
def lib():
    build.build()
    return binding.load()


def host_raycast(name, first=0, count=None):
    case, P, v = rc.view(name)
    vol = tc.model(case)["volume"]
    return binding.tsdf_raycast_pixels(rc.volume_params(binding, case), rc.ray_params(binding, v), P, vol.tsdf, vol.weight,
                                       vol.intensity, first=first, count=count)


@pytest.mark.parametrize("name", rc.TABLE + ("room_color",))
def test_raycast_pixels_gives_the_models_bits(lib, name):
    m = rc.model(name)
    rows, cols = rc.view(name)[2]["shape"]
    maps, listed = host_raycast(name)
    assert maps.shape == (8, rows * cols) and listed == m["n_hits"]
    assert maps.tobytes() == m["maps"].tobytes()
    assert int((maps[6] > 0).sum()) == listed
    # split ranges concatenate to the whole: a ragged first piece, one pixel, the rest
    cuts = [0, 7 * cols + 3, 7 * cols + 4, rows * cols]
    parts = [host_raycast(name, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.concatenate([p[0] for p in parts], axis=1).tobytes() == maps.tobytes()
    assert sum(p[1] for p in parts) == listed
    assert host_raycast(name, 5, 0)[0].shape == (8, 0)
    if name == "room_color":
        inten = maps[7][maps[6] > 0]
        assert inten.min() >= 0 and inten.max() <= 1 and np.ptp(inten) > 0.1
    else:
        assert not maps[7].any()


@pytest.mark.parametrize("name", rc.TABLE)
def test_the_tables_counts_hold(name):
    _, _, _, crossings, listed = rc.VIEWS[name]
    m = rc.model(name)
    assert (int(m["crossing"].sum()), m["n_hits"]) == (crossings, listed)
    assert m["n_no_normal"] == crossings - listed == int((m["reason"] != rm.LISTED).sum())
    assert not (m["crossing"] & m["back_face"]).any()
    valid = m["maps"][6] > 0
    assert int(valid.sum()) == listed and not m["maps"][:, ~valid].any()
    if name == "room_z_far":
        assert abs(float(m["maps"][6].max()) - 2.2375) < 5e-5
    if name == "plane":  # every listed depth is exactly 1.5 and every normal exactly (0, 0, -1)
        assert np.all(m["maps"][6][valid] == np.float32(1.5))
        assert np.all(m["maps"][3][valid] == 0) and np.all(m["maps"][4][valid] == 0) and np.all(m["maps"][5][valid] == -1)
    if name == "plane_reversed":  # all 3 072 rays end on the back-face rule
        assert int(m["back_face"].sum()) == 48 * 64 == 3072
    if name == "odd":
        assert 37 % 8 and 53 % 8 and (37 * 53) % 256
    if name == "holes":  # every crossing lands in n_no_normal
        assert m["n_hits"] == 0 and m["n_no_normal"] == 204


def test_sample_count_is_the_headers():
    assert rm.n_samples(0.25, 6.0, 0.125) == 47 and rm.n_samples(0.25, 2.5, 0.125) == 19
    assert rm.n_samples(0.01, 3.0, 0.03) == 100 and rm.n_samples(0.25, 3.0, 0.1875) == 15


def test_accuracy_on_the_room():
    """Measured: largest distance of a listed hit to the analytic room 0.0201 m, median 0.0002 m; |depth - d4 / 5000|
    99th percentile 0.0169 m; the voxel is 0.0625 m."""
    m = rc.model("room")["maps"]
    valid = m[6] > 0
    dist = tc.room_distance(m[:3][:, valid].astype(np.float64))
    d4, _ = tc.room_frame(*tc.ROOM_FOURTH)
    both = valid & (d4 > 0)
    diff = np.abs(m[6][both].astype(np.float64) - d4[both] / 5000.0)
    voxel = tc.ROOM_VOLUME["voxel"]
    print(f"room: {int(valid.sum())} hits, distance to the analytic room max {dist.max():.4f} median {np.median(dist):.4f}, "
          f"within half a voxel {np.mean(dist < voxel / 2):.4f}; |depth - d4 / 5000| over {int(both.sum())} pixels "
          f"99th percentile {np.percentile(diff, 99):.4f} median {np.median(diff):.4f}")
    assert np.mean(dist < voxel / 2) >= 0.99
    assert both.sum() > 10000 and np.percentile(diff, 99) < voxel / 2


def test_refusals_of_raycast_pixels(lib):
    case, P, v = rc.view("plane")
    vol = tc.model(case)["volume"]
    p, r = rc.volume_params(binding, case), rc.ray_params(binding, v)
    n = vol.tsdf.size
    f, w = np.ascontiguousarray(vol.tsdf).reshape(-1), np.ascontiguousarray(vol.weight).reshape(-1)
    out = np.zeros((8, 48 * 64), np.float32)
    fp, u16, dp = C.POINTER(C.c_float), C.POINTER(C.c_uint16), C.POINTER(C.c_double)
    Pc = np.ascontiguousarray(P, np.float64).reshape(16)

    def call(params=p, ray=r, pose=Pc, tsdf=f, weight=w, intensity=None, first=0, count=48 * 64, o=out):
        return lib.icpk_tsdf_raycast_pixels(None if params is None else C.byref(params), None if ray is None else C.byref(ray),
                                            None if pose is None else pose.ctypes.data_as(dp),
                                            None if tsdf is None else tsdf.ctypes.data_as(fp),
                                            None if weight is None else weight.ctypes.data_as(u16),
                                            None if intensity is None else intensity.ctypes.data_as(fp), first, count,
                                            None if o is None else o.ctypes.data_as(fp))

    assert call() == 432
    for kw in (dict(params=None), dict(ray=None), dict(pose=None), dict(tsdf=None), dict(weight=None), dict(o=None),
               dict(first=-1), dict(count=-1), dict(first=1), dict(first=48 * 64, count=1),
               dict(intensity=np.zeros(n, np.float32)),  # (a plane the volume does not keep)
               dict(pose=np.full(16, np.nan)), dict(pose=np.where(np.arange(16) == 3, np.inf, Pc))):
        assert call(**kw) == binding.E_ARG, kw
    bad = [dict(shape=(0, 64)), dict(shape=(48, -1)), dict(shape=(2048, 1025)), dict(fx=0.0), dict(fx=float("nan")),
           dict(cx=float("inf")), dict(z_near=float("nan")), dict(z_far=float("inf")), dict(step=float("nan")),
           dict(z_near=0.0), dict(z_near=-1.0), dict(z_far=0.25), dict(z_far=0.1), dict(step=-0.1),
           dict(step=2.75 / 4096), dict(min_weight=0), dict(min_weight=65536)]
    for kw in bad:
        assert call(ray=binding.tsdf_raycast_params(**dict(v, **kw))) == binding.E_ARG, kw
    assert call(ray=binding.tsdf_raycast_params(**dict(v, step=2.75 / 4095))) >= 0  # (N = 4096 is still allowed)
    assert call(params=binding.tsdf_params(dims=(0, 4, 4), voxel=0.1, origin=(0, 0, 0), trunc=0.2)) == binding.E_ARG
    # a colour volume wants its intensity plane
    pc = rc.volume_params(binding, "room_color")
    big = np.zeros(64 ** 3, np.float32)
    assert call(params=pc, tsdf=big, weight=np.zeros(64 ** 3, np.uint16), count=1) == binding.E_ARG
    assert call(params=pc, tsdf=big, weight=np.zeros(64 ** 3, np.uint16), intensity=big, count=1) == 0
    # step 0 is trunc / 2
    a = binding.tsdf_raycast_pixels(p, binding.tsdf_raycast_params(**dict(v, step=0.0)), P, f, w)
    b = binding.tsdf_raycast_pixels(p, binding.tsdf_raycast_params(**dict(v, step=0.1875)), P, f, w)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == 432
    d = binding.tsdf_raycast_params()
    assert (d.rows, d.cols, d.z_near, d.z_far, d.step, d.min_weight) == (480, 640, 0.25, 6.0, 0.0, 1)
    assert (d.fx, d.cx) == (np.float32(468.60), np.float32(318.27))
