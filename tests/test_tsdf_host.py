"""The rules of the TSDF volume (K19) without a GPU: icpk_tsdf_voxel_update -- the host half of csrc/tsdf_rule.h, the
header the kernel includes -- against tests/tsdf_model.py bit for bit; the model against an independent float64
implementation; and the model's surface on a plane and on the analytic room."""
import ctypes as C

import numpy as np
import pytest

import tsdf_cases as tc
import tsdf_model
from icp_slam_prototype_amd import binding, build

EPS = 2.0 ** -24  # half an ulp of 1 in float32: the relative error of one rounding


@pytest.fixture(scope="module")
def lib():
    build.build()
    return binding.load()


def params_of(c):
    v = c["volume"]
    return binding.tsdf_params(dims=v["dims"], voxel=v["voxel"], origin=v["origin"], trunc=v["trunc"],
                               max_weight=v.get("max_weight"), flags=binding.TSDF_COLOR if v.get("color") else 0)


@pytest.mark.parametrize("name", tc.SMALL_CASES)
def test_voxel_update_gives_the_models_bits(lib, name):
    c, m = tc.case(name), tc.model(name)
    p = params_of(c)
    n = int(np.prod(c["volume"]["dims"]))
    tsdf, weight = np.zeros(n, np.float32), np.zeros(n, np.uint16)
    inten = np.zeros(n, np.float32) if c["volume"].get("color") else None
    for k, (d, P, img) in enumerate(c["frames"]):
        R, t = binding.tsdf_invert_pose(P)
        Rm, tm = tsdf_model.invert_pose(P)
        assert R.tobytes() == Rm.tobytes() and t.tobytes() == tm.tobytes()
        written = binding.tsdf_voxel_update(p, R, t, d, tsdf, weight, img, inten, fx=c["fx"], cx=c["cx"])
        assert written == m["n_updated"][k] and written > 0
        assert tsdf.tobytes() == m["tsdf"][k].tobytes()
        assert weight.tobytes() == m["weight"][k].tobytes()
        if inten is not None:
            assert inten.tobytes() == m["intensity"][k].tobytes() and inten.max() > 0
    # one voxel at a time is the same function: a few voxels of the last frame again, from the state before it
    if len(c["frames"]) > 1:
        d, P, img = c["frames"][-1]
        R, t = binding.tsdf_invert_pose(P)
        changed = np.flatnonzero(m["weight"][-1].reshape(-1) != m["weight"][-2].reshape(-1))[:50]
        for at in list(changed) + [0, n - 1]:
            f1 = m["tsdf"][-2].reshape(-1)[at:at + 1].copy()
            w1 = m["weight"][-2].reshape(-1)[at:at + 1].copy()
            c1 = None if inten is None else m["intensity"][-2].reshape(-1)[at:at + 1].copy()
            binding.tsdf_voxel_update(p, R, t, d, f1, w1, img, c1, fx=c["fx"], cx=c["cx"], first=int(at), count=1)
            assert f1[0].tobytes() == m["tsdf"][-1].reshape(-1)[at].tobytes() and w1[0] == m["weight"][-1].reshape(-1)[at]


def test_voxel_update_refuses_bad_arguments(lib):
    c = tc.case("boundary")
    p = params_of(c)
    d, P, _ = c["frames"][0]
    R, t = binding.tsdf_invert_pose(P)
    f, w = np.zeros(4, np.float32), np.zeros(4, np.uint16)
    n = int(np.prod(c["volume"]["dims"]))
    with pytest.raises(binding.IcpkError):
        binding.tsdf_voxel_update(p, R, t, d, f, w, fx=64.0, cx=7.5, first=n - 3, count=4)  # past the volume
    with pytest.raises(binding.IcpkError):
        binding.tsdf_voxel_update(p, R, t, d, f, w, intensity=np.zeros(d.shape, np.float32), fx=64.0, cx=7.5)  # no colour volume
    bad = binding.tsdf_params(dims=(0, 4, 4))
    with pytest.raises(binding.IcpkError):
        binding.tsdf_voxel_update(bad, R, t, d, f, w, fx=64.0, cx=7.5)
    with pytest.raises(binding.IcpkError):
        binding.tsdf_invert_pose(np.full((4, 4), np.nan))
    assert f.tobytes() == bytes(16) and not w.any()


def integrate_f64(vol, frames, fx, cx, dq):
    """The rule written the ordinary way in float64: matrix products, np.round.  dq: the bound on the float32 rule's
    error in q.  Returns (tsdf, weight, settled): settled = in no frame did the voxel come so near a decision (q_z = 0,
    a pixel boundary, sdf = -trunc) that an error of dq in q could take it the other way."""
    dx, dy, dz = vol["dims"]
    k, j, i = np.meshgrid(np.arange(dz), np.arange(dy), np.arange(dx), indexing="ij")
    p = (np.stack([i, j, k], -1) + 0.5) * float(np.float32(vol["voxel"])) + np.asarray(vol["origin"], np.float32).astype(np.float64)
    tsdf, weight = np.zeros((dz, dy, dx)), np.zeros((dz, dy, dx), np.int64)
    settled = np.ones((dz, dy, dx), bool)
    trunc = float(np.float32(vol["trunc"]))
    fx, cx = float(np.float32(fx)), float(np.float32(cx))
    for d, P, _ in frames:
        rows, cols = d.shape
        q = (p - P[:3, 3]) @ P[:3, :3]  # R^T (p - t)
        qz = q[..., 2]
        with np.errstate(all="ignore"):
            u = q[..., 0] * fx / qz + cx
            v = q[..., 1] * fx / qz + cx
            col, row = np.floor(u + 0.5), np.floor(v + 0.5)
            inside = (qz > 0) & (col >= 0) & (col < cols) & (row >= 0) & (row < rows)
            depth = d[np.where(inside, row, 0).astype(int), np.where(inside, col, 0).astype(int)]
            sdf = depth / 5000.0 - qz
            ok = inside & (depth != 0) & (sdf >= -trunc)
            f = np.minimum(1.0, sdf / trunc)
            tsdf = np.where(ok, (tsdf * weight + f) / (weight + 1.0), tsdf)
            weight = np.where(ok, np.minimum(weight + 1, vol.get("max_weight", 255)), weight)
            # u = q_x fx / q_z + cx: du <= (fx / q_z) (dq + |q_x| dq / q_z), and three more roundings of u itself
            du = fx / np.abs(qz) * dq * (1 + (np.abs(q[..., 0]) + np.abs(q[..., 1])) / np.abs(qz)) + 4 * EPS * (np.abs(u) + np.abs(v) + 1)
            pix = np.minimum(np.abs(u + 0.5 - np.round(u + 0.5)), np.abs(v + 0.5 - np.round(v + 0.5)))
            sure = (np.abs(qz) > dq) & ((qz < 0) | (pix > du))
            sure &= ~(inside & (depth != 0)) | (np.abs(sdf + trunc) > 2 * dq)
            settled &= sure
    return tsdf, weight, settled


@pytest.mark.parametrize("name", ["room", "odd", "holes", "saturation"])
def test_model_agrees_with_float64_written_the_ordinary_way(name):
    """Roundings counted along the float32 rule, each of relative size EPS; M = a bound on every magnitude met (the
    volume's far corner, the camera centre, the largest depth):
      q    the centre 3, the float pose 1 per entry, each row 3 products, 3 sums: within dq = 12 EPS M;
      sdf  d / scale 1, the difference 1: within 14 EPS M;  f = sdf / trunc 1 more: within 14 EPS M / trunc + EPS;
      mean 3 roundings of numbers <= 1 per frame on top of the mean of the f errors: 3 EPS per frame.
    Voxels that come within those errors of a decision (q_z = 0, a pixel boundary, sdf = -trunc) in some frame are set
    aside -- a few per cent, near the camera, where fx / q_z magnifies dq into a few thousandths of a pixel -- and
    every other voxel must have taken the same decisions."""
    c, m = tc.case(name), tc.model(name)
    vol = c["volume"]
    corner = np.abs(np.asarray(vol["origin"], np.float64)) + np.asarray(vol["dims"]) * vol["voxel"]
    M = corner.sum() + max(np.abs(P[:3, 3]).sum() for _, P, _ in c["frames"]) + 65535 / 5000.0
    ref, wref, settled = integrate_f64(vol, c["frames"], c["fx"], c["cx"], 12 * EPS * M)
    tol = EPS * (14 * M / vol["trunc"] + 1 + 3 * len(c["frames"]))
    assert settled.mean() > 0.9
    assert np.array_equal(m["weight"][-1][settled], wref[settled])
    err = np.abs(m["tsdf"][-1].astype(np.float64) - ref)[settled]
    print(f"{name}: float32 model against float64, max |diff| {err.max():.3g}, tolerance {tol:.3g}, "
          f"{int((~settled).sum())} voxels set aside")
    assert err.max() <= tol
    assert (wref[settled] > 0).sum() > 100


def test_plane_crossings_lie_on_the_plane_with_exact_normals():
    """Constant depth z0, identity pose, dyadic voxel, origin and trunc.  Exact arithmetic puts every crossing at z0:
    sdf is exact (dyadic numbers), t = sdf_V / (sdf_V - sdf_N) and z_V + t voxel = z0.  In float32: f = sdf / trunc rounds
    (EPS each, the first division); f_V and f_N have opposite signs, so their difference has no cancellation and rounds
    once more (EPS); the second division rounds t (EPS): t is within 4 EPS (1 + EPS)^3 of exact, t voxel -- the one
    multiply, exact here since voxel is a power of two, EPS otherwise -- within 5 EPS voxel, and the final sum rounds to
    half an ulp of z0: EPS z0."""
    c, m = tc.case("plane"), tc.model("plane")
    s = m["surface"]
    n = s["points"].shape[1]
    assert n == 80 and (s["axis"] == 2).all()
    bound = EPS * (5.5 * c["volume"]["voxel"] + c["z0"])
    assert np.abs(s["points"][2].astype(np.float64) - c["z0"]).max() <= bound
    assert np.array_equal(s["normals"], np.tile(np.float32([[0], [0], [-1]]), (1, n)))
    # x and y are V's centres, untouched
    cx, cy, _ = m["volume"].centres()
    dx, dy, _ = c["volume"]["dims"]
    assert np.array_equal(s["points"][0], cx[s["voxel"] % dx]) and np.array_equal(s["points"][1], cy[(s["voxel"] // dx) % dy])
    # the crossings on the last x and y layers have no gradient: dropped, not listed
    dv = s["dropped_voxel"]
    assert ((dv % dx) == dx - 1).any() and (((dv // dx) % dy) == dy - 1).any() and s["n_no_normal"] == 40
    e = tc.model("plane_edge")["surface"]
    assert e["points"].shape[1] == 0 and e["n_no_normal"] == 120  # (N on the last z layer: every crossing dropped)


def test_room_surface_lies_on_the_analytic_room():
    """Three frames of the room into 64^3: at least 99 % of the extracted points within one voxel edge of the floor,
    the walls or the sphere.  Measured (every crossing, before the normal rule drops those without a gradient): 3 913
    crossings, 0.026 % beyond one voxel, 0.26 % beyond half a voxel, largest distance 0.071 (at occlusion edges); the
    3 410 listed ones: none beyond half a voxel, largest distance 0.029."""
    m = tc.model("room")
    s = m["surface"]
    voxel = tc.ROOM_VOLUME["voxel"]
    d_all = tc.room_distance(s["crossing_points"])
    d = tc.room_distance(s["points"])
    print(f"room: {d_all.size} crossings, {100 * (d_all > voxel).mean():.3f} % beyond one voxel, "
          f"{100 * (d_all > voxel / 2).mean():.2f} % beyond half a voxel, largest distance {d_all.max():.3f}; "
          f"{d.size} listed, {100 * (d > voxel / 2).mean():.2f} % beyond half a voxel, largest {d.max():.3f}")
    assert d_all.size == 3913 and d.size + s["n_no_normal"] == 3913
    assert (d_all <= voxel).mean() >= 0.99 and (d <= voxel).mean() >= 0.99
    # normals are unit vectors that face the cameras (all three stand near the origin)
    nrm = s["normals"].astype(np.float64)
    assert np.abs(np.linalg.norm(nrm, axis=0) - 1).max() < 4 * EPS * 2
    assert ((-s["points"].astype(np.float64) * nrm).sum(0) > 0).mean() > 0.99
    # the list is ordered by voxel, then axis
    key = s["voxel"].astype(np.int64) * 3 + s["axis"]
    assert (np.diff(key) > 0).all()


def test_boundary_case_meets_its_three_events():
    c = tc.case("boundary")
    v = tsdf_model.Volume(**c["volume"])
    d, P, _ = c["frames"][0]
    _, dbg = v.integrate(d, P, c["fx"], c["cx"], debug=True)
    a = dbg["u"] + np.float32(0.5)
    assert (dbg["front"] & (a == np.floor(a))).sum() >= 100           # centres on a pixel boundary
    assert (dbg["u"] == -0.5).any() and (dbg["u"] == d.shape[1] - 0.5).any()
    assert (dbg["ok"] & (dbg["u"] == -0.5)).any() and not (dbg["ok"] & (dbg["u"] == d.shape[1] - 0.5)).any()
    edge = dbg["seen"] & (dbg["sdf"] == -np.float32(c["volume"]["trunc"]))
    assert edge.any() and dbg["ok"][edge].all()                       # sdf == -trunc is still written
    assert C.sizeof(binding.TsdfParams) == 11 * 4
