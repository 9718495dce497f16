"""K27 on the device: icpk_fern_encode through a real icpk_depth_pyramid_build, icpk_fern_query over databases built with
icpk_fern_add_code, and the harvest of icpk_fern_process over the scene, all against tests/fern_model.py byte for byte;
repeatability (three runs, reset, destroy + create, save / load); what the calls leave alone; ICPK_E_NOT_SET for a stale
code; every ICPK_E_ARG refusal with the database as it was."""
import numpy as np
import pytest

import fern_model as fm
import pyramid_model as pm
import tsdf_cases as tc
from icp_slam_prototype_amd import binding, depth, synth
from icp_slam_prototype_amd.tsdf import TsdfVolume

pytestmark = pytest.mark.gpu

GEOM = {k: tc.ROOM_VOLUME[k] for k in ("dims", "voxel", "origin", "trunc")}
FERNS = [8, 64, 256, 1024]
I4 = np.eye(4)


@pytest.fixture(scope="module")
def ctx():
    with binding.Context(0) as c:
        yield c


def code_of(call, *a, **kw):
    with pytest.raises(binding.IcpkError) as e:
        call(*a, **kw)
    return e.value.code


def images():
    """name -> (level-0 image, the level encoded): the room at levels 0 .. 2, 19 x 27 with a third of the pixels holes (as
    level 1 of 37 x 53), 1 x 1"""
    room = pm.case("room_120x160")[0]
    rng = np.random.default_rng(27)
    holes = rng.integers(800, 21000, (37, 53)).astype(np.uint16)
    holes[rng.random(holes.shape) < 1 / 3] = 0
    return {"room_l0": (room, 0), "room_l1": (room, 1), "room_l2": (room, 2), "holes_19x27": (holes, 1),
            "1x1": (np.full((1, 1), 5000, np.uint16), 0)}


@pytest.mark.parametrize("F", FERNS)
@pytest.mark.parametrize("name", list(images()))
def test_encode_gives_the_models_bytes(ctx, name, F):
    img, l = images()[name]
    shapes = depth.build_pyramid(ctx, img, depth.pyramid_params(levels=l + 1))
    level = depth.pyramid_level(ctx, l)
    assert level.tobytes() == pm.pyramid(img, l + 1)[l].tobytes() and level.shape == shapes[l]
    if name == "holes_19x27":
        assert level.shape == (19, 27) and 0.2 < (level == 0).mean() < 0.45
    binding.fern_create(ctx, *shapes[l], level=l, n_ferns=F, capacity=4)
    mp = fm.params(level=l, n_ferns=F, capacity=4)
    want, wantV = fm.encode(mp, level)
    code, V = binding.fern_encode(ctx)
    assert code.shape == (F // 8,) and code.tobytes() == want.tobytes() and V == wantV
    r = binding.fern_process(ctx, I4, k=1)  # the per-frame call encodes the same code and keeps it
    assert (r["valid"], r["added"], len(r["index"])) == (wantV, 0 if wantV >= F // 2 else -1, 0)
    if r["added"] == 0:
        assert binding.fern_keyframe(ctx, 0)[0].tobytes() == want.tobytes()
    binding.fern_destroy(ctx)


def random_codes(n, F, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 32, (n, F // 8), dtype=np.uint32)


def fill(c, codes, capacity, level_shape=(30, 40), **kw):
    binding.fern_create(c, *level_shape, n_ferns=8 * codes.shape[1], capacity=capacity, **kw)
    for i, code in enumerate(codes):
        assert binding.fern_add_code(c, code, I4) == i


def resident_level2(c, img=None):
    """a pyramid whose level 2 is 30 x 40, and the current code taken from it"""
    depth.build_pyramid(c, pm.case("room_120x160")[0] if img is None else img, depth.pyramid_params(levels=3))


def check_queries(c, codes, query_code=None):
    """fern_query for k = 1, 3, 8 against the model, the query being the context's current code"""
    n = len(codes)
    for k in (1, 3, 8):
        idx, d = binding.fern_query(c, k)
        widx, wd = fm.search(codes, query_code, k)
        assert idx.dtype == d.dtype == np.int32 and len(idx) == min(k, n)
        assert idx.tobytes() == widx.tobytes() and d.tobytes() == wd.tobytes(), (n, k, idx, widx, d, wd)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_query_gives_the_models_lists(ctx, n):
    """wave and workgroup edges; a capacity that is no multiple of 64; k = 1 and 8, and k > n"""
    F = 256
    codes = random_codes(n, F, n)
    fill(ctx, codes, capacity=n + 3 if n != 256 else 256)
    resident_level2(ctx)
    q, _ = binding.fern_encode(ctx)
    # the query's duplicates at 0, n / 2 and n - 1, a keyframe at dissimilarity exactly F, and near misses around them
    codes[[0, n // 2, n - 1]] = q
    if n > 3:
        codes[1] = q ^ np.uint32(0x11111111)  # every nibble differs: diss == F
        codes[n - 2] = q ^ np.uint32(0x00000100)
    binding.fern_reset(ctx)
    for i, code in enumerate(codes):
        assert binding.fern_add_code(ctx, code, I4) == i
    assert binding.fern_count(ctx) == n
    check_queries(ctx, codes, q)
    idx, d = binding.fern_query(ctx, 8)
    assert list(idx[:3]) == sorted({0, n // 2, n - 1})[:3] or n < 3
    assert d[0] == 0
    if n > 3:
        assert int(fm.diss(codes[1], q)) == F
    binding.fern_destroy(ctx)


def test_query_edges(ctx):
    """identical codes: ties resolve by index; every keyframe at dissimilarity F; F = 8 and 1024; an empty database"""
    for F in (8, 1024):
        resident_level2(ctx)
        binding.fern_create(ctx, 30, 40, n_ferns=F, capacity=700)
        q, _ = binding.fern_encode(ctx)
        assert [len(a) for a in binding.fern_query(ctx, 8)] == [0, 0]  # empty: no launch, no keyframe
        same = np.tile(q ^ np.uint32(0x10), (600, 1))
        for code in same:
            binding.fern_add_code(ctx, code, I4)
        idx, d = binding.fern_query(ctx, 8)
        assert idx.tolist() == list(range(8)) and d.tolist() == [F // 8] * 8  # (one nibble of every word differs)
        binding.fern_reset(ctx)
        far = np.tile(~q, (300, 1))  # (~q differs from q in every nibble)
        for code in far:
            binding.fern_add_code(ctx, code, I4)
        idx, d = binding.fern_query(ctx, 8)
        assert idx.tolist() == list(range(8)) and d.tolist() == [F] * 8
        check_queries(ctx, far, q)
        binding.fern_destroy(ctx)


def run_scene(c, count=fm.SCENE_FRAMES, k=3, **kw):
    """the scene's first `count` frames through build + fern_process(pose); the per-frame results and the database"""
    s = fm.scene()
    binding.fern_create(c, 30, 40, **kw)
    out = []
    for i in range(count):
        depth.build_pyramid(c, s["frames"][i], depth.pyramid_params(levels=3))
        out.append(binding.fern_process(c, s["poses"][i], k))
    return out, [binding.fern_keyframe(c, j) for j in range(binding.fern_count(c))]


def blob(results, keyframes):
    return b"".join(r["index"].tobytes() + r["diss"].tobytes() + f"{r['valid']},{r['added']};".encode() for r in results) + \
        b"".join(code.tobytes() + pose.tobytes() for code, pose in keyframes)


@pytest.fixture(scope="module")
def scene_run(ctx):
    return run_scene(ctx)


def test_harvest_gives_the_models_database(ctx, scene_run):
    results, keyframes = scene_run
    db, want = fm.scene_harvest()
    assert [i for i, r in enumerate(results) if r["added"] >= 0] == fm.SCENE_KEYFRAMES
    for i, (r, w) in enumerate(zip(results, want)):
        assert (r["added"], r["valid"]) == (w["added"], w["valid"]), i
        assert r["index"].tobytes() == w["index"].tobytes() and r["diss"].tobytes() == w["diss"].tobytes(), i
    assert len(keyframes) == len(db.codes) == 6
    for (code, pose), wc, wp in zip(keyframes, db.codes, db.poses):
        assert code.tobytes() == wc.tobytes() and pose.tobytes() == wp.tobytes()
    # the queries: fresh renders of the same poses find a keyframe at most 4 frames away, below the harvest bar
    s = fm.scene()
    for i in range(0, fm.SCENE_FRAMES, 4):
        depth.build_pyramid(ctx, s["queries"][i], depth.pyramid_params(levels=3))
        r = binding.fern_process(ctx, None, 3)
        w = db.process(fm.scene_levels("queries")[i], None, 3)
        assert r["added"] == -1 and r["index"].tobytes() == w["index"].tobytes() and r["diss"].tobytes() == w["diss"].tobytes()
        assert abs(fm.SCENE_KEYFRAMES[r["index"][0]] - i) <= fm.SCENE_MAX_GAP and r["diss"][0] <= 51
    assert binding.fern_count(ctx) == 6


def test_a_full_database_and_a_covered_frame_add_nothing(ctx):
    results, keyframes = run_scene(ctx, capacity=3)
    assert [i for i, r in enumerate(results) if r["added"] >= 0] == fm.SCENE_KEYFRAMES[:3] and len(keyframes) == 3
    assert binding.fern_count(ctx) == 3  # full: fern_process goes on without an error ...
    assert code_of(binding.fern_add, ctx, I4) == binding.E_ARG  # ... fern_add and fern_add_code refuse
    assert code_of(binding.fern_add_code, ctx, keyframes[0][0], I4) == binding.E_ARG
    assert [binding.fern_keyframe(ctx, j)[0].tobytes() for j in range(3)] == [k[0].tobytes() for k in keyframes]
    # a covered lens: V = 0 < min_valid keeps it out of an empty database too
    binding.fern_create(ctx, 30, 40)
    depth.build_pyramid(ctx, np.zeros(tc.ROOM_SHAPE, np.uint16), depth.pyramid_params(levels=3))
    r = binding.fern_process(ctx, I4)
    assert (r["valid"], r["added"], binding.fern_count(ctx)) == (0, -1, 0)
    binding.fern_create(ctx, 30, 40, min_valid=0)
    assert binding.fern_process(ctx, I4)["added"] == 0  # (min_valid is what kept it out)


def test_three_runs_reset_and_recreate_give_the_same_bytes(ctx, scene_run):
    count = 12
    first = run_scene(ctx, count)
    short = blob(*first)
    assert blob(first[0], []) == blob(scene_run[0][:count], [])  # (a frame's result does not depend on what follows)
    assert short == blob(*run_scene(ctx, count)) == blob(*run_scene(ctx, count))
    with binding.Context(0) as fresh:
        assert blob(*run_scene(fresh, count)) == short
    # reset: an empty database that harvests as a new one does
    s = fm.scene()
    binding.fern_reset(ctx)
    assert binding.fern_count(ctx) == 0
    out = []
    for i in range(count):
        depth.build_pyramid(ctx, s["frames"][i], depth.pyramid_params(levels=3))
        out.append(binding.fern_process(ctx, s["poses"][i], 3))
    assert blob(out, [binding.fern_keyframe(ctx, j) for j in range(binding.fern_count(ctx))]) == short
    # destroy, then create with other parameters and back
    binding.fern_destroy(ctx)
    assert code_of(binding.fern_count, ctx) == binding.E_NOT_SET
    run_scene(ctx, 4, n_ferns=64)
    assert blob(*run_scene(ctx, count)) == short


def test_save_and_load_round_trip(ctx, tmp_path):
    s = fm.scene()
    reloc = depth.Relocaliser(ctx, (30, 40))
    for i in range(12):
        depth.build_pyramid(ctx, s["frames"][i], depth.pyramid_params(levels=3))
        reloc.process(s["poses"][i])
    assert reloc.count == 3
    depth.build_pyramid(ctx, s["queries"][7], depth.pyramid_params(levels=3))
    want = reloc.process(None, k=3)
    assert [p.tobytes() for p in want["poses"]] == [s["poses"][fm.SCENE_KEYFRAMES[j]].tobytes() for j in want["index"]]
    path = str(tmp_path / "ferns.npz")
    reloc.save(path)
    before = [binding.fern_keyframe(ctx, j) for j in range(3)]
    with binding.Context(0) as other:
        again = depth.Relocaliser.load(other, path)
        assert again.count == 3 and bytes(again.params) == bytes(reloc.params)
        assert blob([], [binding.fern_keyframe(other, j) for j in range(3)]) == blob([], before)
        depth.build_pyramid(other, s["queries"][7], depth.pyramid_params(levels=3))
        got = again.process(None, k=3)
        assert got["index"].tobytes() == want["index"].tobytes() and got["diss"].tobytes() == want["diss"].tobytes()
        assert [p.tobytes() for p in got["poses"]] == [p.tobytes() for p in want["poses"]]


def snapshot(c, levels):
    """what the fern calls must leave alone: the clouds, the associations, the maps, the pyramid and its intensity"""
    idx, dist = c.get_associations()
    view = c.tsdf_get_raycast()
    return [c.get_source().tobytes(), c.get_target().tobytes(), c.get_target_normals().tobytes(), idx.tobytes(), dist.tobytes()] + \
        [view[k].tobytes() for k in ("points", "normals", "depth", "intensity")] + \
        [depth.pyramid_level(c, l).tobytes() for l in range(levels)] + [binding.pyramid_intensity(c, l).tobytes() for l in range(levels)]


def database(c):
    return [binding.fern_count(c)] + [blob([], [binding.fern_keyframe(c, j)]) for j in range(binding.fern_count(c))]


def test_the_context_is_left_alone_and_refusals_leave_the_database(ctx):
    c = tc.case("room")
    frames = c["frames"]
    vol = TsdfVolume(ctx, **GEOM, fx=tc.ROOM_FX, cx=tc.ROOM_CX)
    for d, P, _ in frames:
        vol.integrate(d, P)
    vol.raycast(frames[2][1], shape=tc.ROOM_SHAPE, step=0.125)
    ctx.backproject_with_normals(frames[2][0], fx=tc.ROOM_FX, cx=tc.ROOM_CX)
    ctx.set_source(synth.backproject(frames[1][0], None, tc.ROOM_FX, tc.ROOM_CX))
    ctx.nn()
    inten = tc.room_intensity(*tc.ROOM_MOTIONS[1])
    depth.build_pyramid(ctx, frames[1][0], depth.pyramid_params(levels=3), intensity=inten)
    before = snapshot(ctx, 3)
    binding.fern_create(ctx, 30, 40, capacity=5)
    code, V = binding.fern_encode(ctx)
    assert binding.fern_add(ctx, frames[1][1]) == 0
    binding.fern_process(ctx, frames[1][1], 8)
    binding.fern_query(ctx, 8)
    binding.fern_add_code(ctx, ~code, I4)
    binding.fern_keyframe(ctx, 1)
    binding.fern_reset(ctx)
    binding.fern_process(ctx, frames[1][1], 1)
    assert binding.fern_count(ctx) == 1
    binding.fern_add_code(ctx, ~code, frames[0][1])
    assert snapshot(ctx, 3) == before
    # a pyramid build leaves the database alone and only invalidates the current code
    db = database(ctx)
    depth.build_pyramid(ctx, frames[2][0], depth.pyramid_params(levels=3))
    assert database(ctx) == db
    assert code_of(binding.fern_query, ctx, 3) == binding.E_NOT_SET and code_of(binding.fern_add, ctx, I4) == binding.E_NOT_SET
    assert database(ctx) == db
    code2, _ = binding.fern_encode(ctx)
    assert code2.tobytes() == fm.encode(fm.params(), depth.pyramid_level(ctx, 2))[0].tobytes()
    assert len(binding.fern_query(ctx, 3)[0]) == 2
    # every ICPK_E_ARG refusal leaves the database, and the current code, as they were
    bad = np.eye(4)
    bad[1, 3] = np.nan
    for call, args in ((binding.fern_query, (ctx, 0)), (binding.fern_query, (ctx, 9)), (binding.fern_process, (ctx, None, 0)), (binding.fern_process, (ctx, None, 9)),
                       (binding.fern_process, (ctx, bad, 3)), (binding.fern_add, (ctx, bad)), (binding.fern_add_code, (ctx, code, bad)),
                       (binding.fern_keyframe, (ctx, 2)), (binding.fern_keyframe, (ctx, -1))):
        assert code_of(call, *args) == binding.E_ARG, (call.__name__, args)
    lib, h = ctx._lib, ctx._h
    assert lib.icpk_fern_query(h, 3, None, None, None) == binding.E_ARG
    assert lib.icpk_fern_process(h, None, 3, None, None, None, None, None) == binding.E_ARG
    assert lib.icpk_fern_add(h, None, None) == binding.E_ARG and lib.icpk_fern_add_code(h, None, None, None) == binding.E_ARG
    assert lib.icpk_fern_count(None) == binding.E_ARG and lib.icpk_fern_create(None, None, 30, 40) == binding.E_ARG
    for fields in (dict(n_ferns=12), dict(capacity=0), dict(d_min=7, d_max=7), dict(level=8)):
        assert code_of(binding.fern_create, ctx, 30, 40, **fields) == binding.E_ARG
    assert code_of(binding.fern_create, ctx, 0, 40) == binding.E_ARG
    assert database(ctx) == db and binding.fern_query(ctx, 3)[0].tolist() == [0, 1]
    # a level the pyramid lacks; a resident level of another shape
    depth.build_pyramid(ctx, frames[2][0], depth.pyramid_params(levels=2))
    assert code_of(binding.fern_encode, ctx) == binding.E_ARG and code_of(binding.fern_process, ctx, None, 3) == binding.E_ARG
    depth.build_pyramid(ctx, frames[2][0][:100], depth.pyramid_params(levels=3))
    assert code_of(binding.fern_encode, ctx) == binding.E_ARG and code_of(binding.fern_process, ctx, I4, 3) == binding.E_ARG
    assert database(ctx) == db
    binding.fern_destroy(ctx)
    for call, args in ((binding.fern_encode, (ctx,)), (binding.fern_query, (ctx, 3)), (binding.fern_process, (ctx, None, 3)), (binding.fern_reset, (ctx,)),
                       (binding.fern_add, (ctx, I4)), (binding.fern_add_code, (ctx, code, I4)), (binding.fern_keyframe, (ctx, 0))):
        assert code_of(call, *args) == binding.E_NOT_SET, call.__name__
    with binding.Context(0) as bare:  # a database, but no pyramid
        binding.fern_create(bare, 30, 40)
        assert code_of(binding.fern_encode, bare) == binding.E_NOT_SET and code_of(binding.fern_process, bare, None, 3) == binding.E_NOT_SET
        assert code_of(binding.fern_query, bare, 3) == binding.E_NOT_SET
