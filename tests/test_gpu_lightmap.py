"""Lightmap baking on the GPU (include/rt_mi355x.h: rt_lightmap_*, the kernels of csrc/rt_lightmap.hip). rt_lightmap_texels is compared
with the numpy model of tests/test_lightmap.py (owner_model, texel_model), rt_lightmap_bake with its chain: the model's texels and states
through the library's own gather (Scene.gather_paths over the covered texels), then resolve_model and dilate_model; once the gather is the
CPU oracle's (tests/test_gather.py: gather_model over OracleScene.trace_paths). Every comparison is assert_array_equal."""
import ctypes as C

import numpy as np
import pytest

from rtamd import abi, bake, scenes
from rtamd.renderer import Lightmap, Scene
from test_lightmap import (CORNELL_ATLASES, CORNELL_ORACLE_ATLAS, NONE, diagonal_quad_uvs, dilate_model, entry_states, jittered_grid_uvs,
                           owner_model, resolve_model, stats_model, texel_model)

pytestmark = pytest.mark.gpu
f32 = np.float32
ATLASES = [(1, 1), (7, 5), (64, 64), (65, 33), (256, 256)]
QNAN = 0x7FC00000


@pytest.fixture(scope="module")
def gpu(rtlib):
    assert rtlib.rt_device_count() > 0, "GPU tests need a device; the product has no CPU fallback"
    yield 0
    for s in _SCENES.values():
        s.close()
    _SCENES.clear()


_SCENES, _DESCS = {}, {}


def synthetic_desc(n_tris, seed=1):
    """n_tris random triangles with smooth random vertex normals, dealt to two instances under different rotations and non-uniform scales,
    so that the world vertices and the normal matrix both matter. What the lightmap UVs of the synthetic cases are laid over."""
    key = (n_tris, seed)
    if key not in _DESCS:
        g = np.random.default_rng(seed)
        b = scenes.SceneBuilder(f"lm{n_tris}")
        mat = b.add_material(scenes.Material(color=(0.7, 0.6, 0.5)))
        xfs = [scenes.trs((0.3, -0.2, 0.1), scenes.quat_axis_angle((1, 2, 3), 0.7), (1.0, 2.0, 0.5)),
               scenes.trs((-1.0, 0.5, 2.0), scenes.quat_axis_angle((0, 1, 0), -1.1), (0.25, 1.5, 3.0))]
        for k in range(2):
            t = (n_tris + 1 - k) // 2
            if t == 0:
                continue
            pos = g.uniform(-1, 1, size=(3 * t, 3)) + np.repeat(g.uniform(-3, 3, size=(t, 3)), 3, 0)
            nrm = g.normal(size=(3 * t, 3))
            nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
            mesh = b.add_mesh(pos, nrm, g.uniform(size=(3 * t, 2)), np.arange(3 * t).reshape(t, 3))
            b.add_instance(mesh, mat, xfs[k])
        _DESCS[key] = b.build()
        assert _DESCS[key].n_triangles == n_tris
    return _DESCS[key]


def named_desc(name):
    if name not in _DESCS:
        _DESCS[name] = scenes.get_scene("atrium", coarse=True) if name == "atrium" else scenes.get_scene(name)
    return _DESCS[name]


def device_scene(key, sd, gpu):
    if key not in _SCENES:
        _SCENES[key] = Scene(sd, device=gpu)
    return _SCENES[key]


# ---- the synthetic UV sets, in units of the atlas -------------------------------------------------------------------------------------------
def mixed_uvs(W, H):
    """Twelve triangles, the low indices on top: inside one texel and off its centre; around exactly one centre; two without area; a NaN
    and an infinite coordinate; one corner at 1e30 (finite in texel space: a sliver across the atlas, its box clamped far outside); three
    corners at +-1e30 (every edge value overflows); two that overlap, one per winding; one from -0.3 to 1.4, its box clamped on all four
    sides; and one over the whole atlas, which takes what the others leave."""
    tx, ty = W // 2, H // 2
    t = lambda pts: [((tx + x) / W, (ty + y) / H) for x, y in pts]  # noqa: E731
    return np.array([
        t([(0.1, 0.1), (0.4, 0.1), (0.1, 0.4)]),
        t([(0.1, 0.1), (1.2, 0.1), (0.1, 1.2)]) if W > 1 else t([(0.1, 0.1), (0.9, 0.1), (0.1, 0.95)]),
        [(0.25, 0.25), (0.5, 0.5), (0.75, 0.75)],
        [(0.5, 0.25), (0.5, 0.25), (0.75, 0.5)],
        [(0.1, 0.1), (np.nan, 0.2), (0.3, 0.9)],
        [(0.1, 0.1), (0.9, np.inf), (0.3, 0.9)],
        [(0.1, 0.1), (0.9, 0.2), (1e30, 0.9)],
        [(1e30, 1e30), (-1e30, -1e30), (1e30, -1e30)],
        [(0.05, 0.1), (0.6, 0.15), (0.2, 0.7)],
        [(0.1, 0.05), (0.25, 0.8), (0.7, 0.3)],
        [(-0.3, -0.3), (-0.3, 1.4), (1.4, -0.3)],
        [(0.0, 0.0), (2.0, 0.0), (0.0, 2.0)],
    ], f32)


def uv_case(name, W, H):
    if name == "mixed":
        return mixed_uvs(W, H)
    if name == "mixed_reversed":
        return np.ascontiguousarray(mixed_uvs(W, H)[::-1])
    if name == "mixed_without_the_whole":
        return np.ascontiguousarray(mixed_uvs(W, H)[:-1][::-1])  # the clamped triangle first, then the overlapping pair in the other order
    if name == "whole":
        return mixed_uvs(W, H)[-1:]
    if name == "clamped":
        return mixed_uvs(W, H)[-2:-1]
    if name in ("diagonal01", "diagonal10"):
        return diagonal_quad_uvs((0, 1) if name == "diagonal01" else (1, 0))
    if name == "grid":
        return jittered_grid_uvs(W, H, 7, lo=(0.052 * W, 0.055 * H), hi=(0.945 * W, 0.938 * H))[0]
    raise KeyError(name)


UV_CASES = ["mixed", "mixed_reversed", "mixed_without_the_whole", "whole", "clamped", "diagonal01", "diagonal10", "grid"]


def assert_texels(lm, sd, uv, W, H, what):
    """rt_lightmap_texels against the model, all three planes; -> the model's (owner, pos, normal)"""
    owner = owner_model(uv, W, H)
    pos, nrm = texel_model(sd, uv, W, H, owner)
    got = lm.texels()
    np.testing.assert_array_equal(got["tri"].reshape(-1), owner, err_msg=f"{what}: tri")
    np.testing.assert_array_equal(got["pos"].reshape(-1, 3), pos, err_msg=f"{what}: pos")
    np.testing.assert_array_equal(got["normal"].reshape(-1, 3), nrm, err_msg=f"{what}: normal")
    empty = owner == NONE
    assert (got["pos"].reshape(-1, 3)[empty].view(np.uint32) == QNAN).all() and (got["normal"].reshape(-1, 3)[empty].view(np.uint32) == 0).all()
    return owner, pos, nrm


# ---- 1. texels against the model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", UV_CASES)
@pytest.mark.parametrize("atlas", ATLASES, ids=lambda a: f"{a[0]}x{a[1]}")
def test_texels_of_the_synthetic_cases_equal_the_model(gpu, atlas, name):
    W, H = atlas
    uv = uv_case(name, W, H)
    sd = synthetic_desc(len(uv))
    lm = Lightmap(device_scene(("synthetic", len(uv)), sd, gpu), uv, W, H)
    owner, _, _ = assert_texels(lm, sd, uv, W, H, f"{name} {W}x{H}")
    lm.close()
    o = owner.reshape(H, W)
    if name == "whole":
        assert (o == 0).all()  # at 256 x 256 the box is cut into row bands and every lane strides many times
    if name == "mixed":
        assert (o != NONE).all() and o[H // 2, W // 2] == 1
        assert not np.isin(o, [0, 2, 3, 4, 5, 7]).any()  # off the centre, without area, not finite, overflowing to NaN
        if W >= 64:
            assert (o == 1).sum() == 1 and (o == 8).any() and (o == 9).any() and (o == 10).any() and (o == 11).any()
    if name == "mixed_without_the_whole" and W >= 64:
        assert (o == NONE).any()
        assert o[0, 0] == 0 and o[0, W - 1] == 0 and o[H - 1, 0] == 0  # the clamped triangle reaches three corners of the atlas
    if name == "grid" and W >= 64:
        assert len(np.unique(owner)) > 100
    if name.startswith("diagonal") and W == H:
        assert (np.diag(o) == 0).all()


@pytest.mark.parametrize("name,atlas,gutter", [("cornell", CORNELL_ATLASES[0], 1), ("cornell", CORNELL_ATLASES[1], 1),
                                               ("cornell", CORNELL_ORACLE_ATLAS[:2], CORNELL_ORACLE_ATLAS[2]), ("cube", (64, 64), 1),
                                               ("cube", (65, 33), 1), ("atrium", (1024, 1024), 0), ("empty", (7, 5), 1), ("empty", (64, 64), 1)])
def test_texels_of_the_scenes_under_the_grid_unwrap_equal_the_model(gpu, name, atlas, gutter):
    W, H = atlas
    sd = named_desc(name)
    uv = bake.triangle_grid_uvs(sd.n_triangles, W, H, gutter)
    lm = Lightmap(device_scene(name, sd, gpu), uv, W, H)
    owner, pos, nrm = assert_texels(lm, sd, uv, W, H, f"{name} {W}x{H}")
    lm.close()
    if name == "empty":
        assert (owner == NONE).all()
    else:
        assert len(np.unique(owner[owner != NONE])) == sd.n_triangles
        assert np.isfinite(nrm).all() and np.allclose(np.linalg.norm(nrm[owner != NONE].astype(np.float64), axis=1), 1.0, atol=1e-6)


def test_texels_in_the_device_form_with_outputs_left_out(gpu):
    import torch
    W, H = 65, 33
    uv = uv_case("mixed_without_the_whole", W, H)
    sd = synthetic_desc(len(uv))
    lm = Lightmap(device_scene(("synthetic", len(uv)), sd, gpu), uv, W, H, max_repeats=2)
    owner = owner_model(uv, W, H)
    pos, nrm = texel_model(sd, uv, W, H, owner)
    st = torch.cuda.Stream(device=0)
    for want in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        tri = torch.full((H * W,), 0x55555555, dtype=torch.int32, device="cuda")
        p, n = (torch.full((H * W, 3), 7.0, dtype=torch.float32, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        lm.texels_device(tri.data_ptr() * want[0], p.data_ptr() * want[1], n.data_ptr() * want[2], stream=st.cuda_stream)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(tri.cpu().numpy().view(np.uint32), owner if want[0] else np.full(H * W, 0x55555555, np.uint32))
        np.testing.assert_array_equal(p.cpu().numpy(), pos if want[1] else np.full((H * W, 3), 7.0, f32))
        np.testing.assert_array_equal(n.cpu().numpy(), nrm if want[2] else np.full((H * W, 3), 7.0, f32))
    with pytest.raises(abi.RtError) as e:
        lm.texels_device()
    assert e.value.status == abi.RT_ERR_INVALID
    lm.close()


# ---- 2. bake against its chain ------------------------------------------------------------------------------------------------------------------
SAMPLES, DEPTH, SEED = 2, 5, 11
_GATHERED = {}


def chain(gather, sd, uv, W, H, samples, depth, seed, repeats, rr_start, dilate, key=None):
    """The bake as the contract states it: the model's texels and states, `gather` (Scene.gather_paths or a model of it) over the entries with
    a finite position and normal, the model's resolve and dilation. -> (rgba (H, W, 4), stats). key: the gather's outputs are kept under it."""
    owner = owner_model(uv, W, H)
    if key is None or key not in _GATHERED:
        pos, nrm = texel_model(sd, uv, W, H, owner)
        state = entry_states(W * H, repeats, seed)
        epos, enrm = np.repeat(pos, repeats, 0), np.repeat(nrm, repeats, 0)
        ok = np.isfinite(epos).all(1) & np.isfinite(enrm).all(1)
        assert not ok[np.repeat(owner == NONE, repeats)].any()
        out = gather(epos[ok], enrm[ok], state[ok], depth, samples=samples, rr_start=rr_start)
        rad, rays = np.full((W * H * repeats, 3), np.nan, f32), np.full(W * H * repeats, NONE, np.uint32)
        rad[ok], rays[ok] = out["radiance"], out["rays"]
        if key is None:
            return finish(owner, rad, rays, repeats, W, H, dilate)
        _GATHERED[key] = (rad, rays)
    return finish(owner, *_GATHERED[key], repeats, W, H, dilate)


def finish(owner, rad, rays, repeats, W, H, dilate):
    rgba = dilate_model(resolve_model(owner, rad, rays, repeats).reshape(H, W, 4), dilate)
    return rgba, stats_model(owner, rays, rgba, repeats)


@pytest.fixture(scope="module")
def cornell(gpu):
    """the Cornell box, its unwrap on the first of CORNELL_ATLASES and a lightmap with room for three repeats, shared by the bake tests"""
    W, H = CORNELL_ATLASES[0]
    sd = named_desc("cornell")
    uv = bake.triangle_grid_uvs(sd.n_triangles, W, H)
    s = device_scene("cornell", sd, gpu)
    lm = Lightmap(s, uv, W, H, max_repeats=3)
    yield sd, s, uv, W, H, lm
    lm.close()


@pytest.mark.parametrize("dilate", [0, 1, 4])
@pytest.mark.parametrize("rr_start", [0, 2])
@pytest.mark.parametrize("repeats", [1, 3])
def test_a_bake_is_its_chain_over_the_librarys_own_gather(cornell, repeats, rr_start, dilate):
    sd, s, uv, W, H, lm = cornell
    want, stats = chain(s.gather_paths, sd, uv, W, H, SAMPLES, DEPTH, SEED, repeats, rr_start, dilate, key=("cornell", repeats, rr_start))
    got = lm.bake(SAMPLES, DEPTH, SEED, repeats=repeats, rr_start=rr_start, dilate=dilate)  # repeats 1 < max_repeats 3 too
    np.testing.assert_array_equal(got["rgba"], want)
    assert got["stats"] == stats
    a = want[..., 3]
    assert stats["covered"] == stats["sampled"] == (a == 1).sum() > 116 and (want[a == 1, :3] > 0).any() and stats["rays"] > stats["sampled"] * SAMPLES
    assert (stats["filled"] > 0) == (dilate > 0)


def test_a_bake_is_its_chain_over_the_cpu_oracles_gather(gpu, oracle):
    from test_gather import gather_model
    W, H, gutter = CORNELL_ORACLE_ATLAS
    sd = named_desc("cornell")
    uv = bake.triangle_grid_uvs(sd.n_triangles, W, H, gutter)
    osc = oracle.OracleScene(sd)
    model = lambda pos, nrm, state, depth, samples, rr_start: gather_model(osc.trace_paths, pos, nrm, state, depth, samples, rr_start)  # noqa: E731
    want, stats = chain(model, sd, uv, W, H, 2, 3, 5, 2, 0, 1)
    lm = Lightmap(device_scene("cornell", sd, gpu), uv, W, H, max_repeats=2)
    got = lm.bake(2, 3, 5, repeats=2, dilate=1)
    lm.close()
    np.testing.assert_array_equal(got["rgba"], want)
    assert got["stats"] == stats and stats["sampled"] >= sd.n_triangles and (want[..., :3] > 0).any()


def test_texels_of_a_mesh_with_zero_normals_are_covered_not_sampled_and_filled(gpu):
    sd0 = named_desc("cornell")
    W, H = CORNELL_ATLASES[0]
    uv = bake.triangle_grid_uvs(sd0.n_triangles, W, H)
    inst = 2
    verts = np.unique(np.asarray(sd0.indices)[np.asarray(sd0.tri_instance) == inst])
    normals = np.array(sd0.normals, f32, copy=True)
    normals[verts] = 0.0
    sd = sd0.updated(normals=normals)
    s = Scene(sd, device=gpu)
    lm = Lightmap(s, uv, W, H)
    owner, _, nrm = assert_texels(lm, sd, uv, W, H, "zero normals")
    dark = (owner != NONE) & np.isin(owner, np.flatnonzero(np.asarray(sd.tri_instance) == inst))
    assert dark.sum() >= 2 and np.isnan(nrm[dark]).all() and np.isfinite(nrm[~dark]).all()
    for dilate in (0, 4):
        want, stats = chain(s.gather_paths, sd, uv, W, H, SAMPLES, DEPTH, SEED, 1, 0, dilate, key="zero normals")
        got = lm.bake(SAMPLES, DEPTH, SEED, dilate=dilate)
        np.testing.assert_array_equal(got["rgba"], want)
        assert got["stats"] == stats and stats["covered"] - stats["sampled"] == dark.sum()
        a = got["rgba"][..., 3].reshape(-1)
        assert (a[dark] != 1.0).all() and ((a[dark] == 0.5).any() if dilate else (a[dark] == 0.0).all())
    lm.close(), s.close()


def test_the_device_form_on_a_stream_with_stats_equals_the_host_form(cornell):
    import torch
    sd, s, uv, W, H, lm = cornell
    host = lm.bake(SAMPLES, DEPTH, SEED, repeats=3, rr_start=2, dilate=3)
    st = torch.cuda.Stream(device=0)
    for want_stats in (True, False):
        rgba = torch.full((H, W, 4), 7.0, dtype=torch.float32, device="cuda")
        stats = torch.full((3,), 0x5555555555555555, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        lm.bake_device(rgba.data_ptr(), SAMPLES, DEPTH, SEED, repeats=3, rr_start=2, dilate=3, d_stats=stats.data_ptr() if want_stats else 0,
                       stream=st.cuda_stream)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(rgba.cpu().numpy(), host["rgba"])
        words = stats.cpu().numpy().view(np.uint32)
        if want_stats:
            got = {"covered": int(words[0]), "sampled": int(words[1]), "filled": int(words[2]), "rays": int(stats.cpu().numpy().view(np.uint64)[2])}
            assert got == host["stats"] and words[3] == 0
        else:
            assert (words == 0x55555555).all()


def test_one_seed_gives_one_image_and_another_seed_another(cornell):
    sd, s, uv, W, H, lm = cornell
    a, b = lm.bake(SAMPLES, DEPTH, SEED, repeats=2, dilate=2), lm.bake(SAMPLES, DEPTH, SEED, repeats=2, dilate=2)
    c = lm.bake(SAMPLES, DEPTH, SEED + 1, repeats=2, dilate=2)
    np.testing.assert_array_equal(a["rgba"], b["rgba"])
    assert a["stats"] == b["stats"] and not np.array_equal(a["rgba"], c["rgba"])
    np.testing.assert_array_equal(a["rgba"][..., 3], c["rgba"][..., 3])  # what is sampled and filled does not depend on the seed


def test_repeats_above_max_repeats_and_bad_parameters_are_refused(cornell):
    sd, s, uv, W, H, lm = cornell
    for kw, word in (({"repeats": 4}, "max_repeats"), ({"repeats": 0}, "repeats"), ({"dilate": 17}, "dilate")):
        with pytest.raises(abi.RtError) as e:
            lm.bake(SAMPLES, DEPTH, SEED, **kw)
        assert e.value.status == abi.RT_ERR_INVALID and word in str(e.value)
    for args in ((0, DEPTH), (SAMPLES, 0)):
        with pytest.raises(abi.RtError) as e:
            lm.bake(*args, SEED)
        assert e.value.status == abi.RT_ERR_INVALID
    p = abi.rt_lightmap_params(SAMPLES, DEPTH, 0, 1, SEED, 0)
    assert lm._lib.rt_lightmap_bake(lm.h, C.byref(p), None, None) == abi.RT_ERR_INVALID
    assert lm._lib.rt_lightmap_texels(lm.h, None, None, None) == abi.RT_ERR_INVALID
    assert lm.bake(SAMPLES, DEPTH, SEED, repeats=3)["stats"]["sampled"] > 0  # max_repeats itself is allowed


# ---- 3. scenes that move, lightmaps that come and go ----------------------------------------------------------------------------------------------
def test_an_update_waits_for_a_pending_bake_and_the_next_bake_sees_the_moved_scene(gpu):
    import torch
    from test_scene_update import spin_about_centre
    sd = named_desc("cornell")
    W, H = CORNELL_ATLASES[0]
    uv = bake.triangle_grid_uvs(sd.n_triangles, W, H)
    s = Scene(sd, device=gpu, updatable=True)
    lm = Lightmap(s, uv, W, H, max_repeats=2)
    assert_texels(lm, sd, uv, W, H, "updatable, before")
    before = lm.bake(SAMPLES, DEPTH, SEED, repeats=2, dilate=2)
    st = torch.cuda.Stream(device=0)
    rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    tri = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    pos = torch.zeros((H * W, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        torch.cuda._sleep(200_000_000)  # ~0.1 s of spinning in front of the bake
    lm.bake_device(rgba.data_ptr(), SAMPLES, DEPTH, SEED, repeats=2, dilate=2, stream=st.cuda_stream)
    lm.texels_device(tri.data_ptr(), pos.data_ptr(), 0, stream=st.cuda_stream)  # launches no gather: its own record of the scene's event
    s.update(instances=spin_about_centre(sd, 25.0))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(rgba.cpu().numpy(), before["rgba"])
    old_owner = owner_model(uv, W, H)
    np.testing.assert_array_equal(pos.cpu().numpy(), texel_model(sd, uv, W, H, old_owner)[0])
    assert_texels(lm, s.desc, uv, W, H, "updatable, after")
    fresh = Scene(s.desc, device=gpu)
    lm2 = Lightmap(fresh, uv, W, H, max_repeats=2)
    after, moved = lm.bake(SAMPLES, DEPTH, SEED, repeats=2, dilate=2), lm2.bake(SAMPLES, DEPTH, SEED, repeats=2, dilate=2)
    np.testing.assert_array_equal(after["rgba"], moved["rgba"])
    assert after["stats"] == moved["stats"] and not np.array_equal(after["rgba"], before["rgba"])
    lm2.close(), lm.close(), fresh.close(), s.close()


def test_a_second_lightmap_on_a_static_scene_leaves_the_first_alone(cornell):
    sd, s, uv, W, H, lm = cornell
    first = lm.texels()
    other = Lightmap(s, bake.triangle_grid_uvs(sd.n_triangles, 65, 33), 65, 33)
    other.bake(1, 2, 3)
    other.close()
    again = lm.texels()
    for k in ("tri", "pos", "normal"):
        np.testing.assert_array_equal(first[k], again[k])
