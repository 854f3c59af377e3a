"""Irradiance probe volumes on the GPU (include/rt_mi355x.h: rt_probe_volume_*, the kernels of csrc/rt_probe_volume.hip), bit for bit
against the numpy model of tests/test_probe_volume.py: rt_probe_volume_entries against entries_model, rt_probe_volume_bake against
bake_model around the CPU oracle's path tracer (OracleScene.trace_paths), rt_probe_volume_sample against sample_model on baked and on
synthetic tables. Every comparison is assert_array_equal. The shapes are the smallest that reach each branch."""
import ctypes as C

import numpy as np
import pytest

from rtamd import abi, bake, scenes
from rtamd.renderer import ProbeVolume, Scene
from test_probe_volume import (bake_model, contract_range_model, entries_model, fallback_state, probe_positions, sample_model)

pytestmark = pytest.mark.gpu
f32 = np.float32
DEPTH, SEED, MAX_DIRS = 5, 11, 64
# (origin, spacing, count) per scene: 3 x 2 x 2 probes, inside the Cornell box, among the tables, and anywhere in the empty scene
GRIDS = {"cornell": ((-0.7, -0.3, -0.5), (0.7, 0.8, 1.0), (3, 2, 2)),
         "tables": None,  # fitted to the bounds (grid_of)
         "empty": ((0.0, 1.0, -2.0), (0.5, 0.25, 3.0), (3, 2, 2))}


@pytest.fixture(scope="module")
def gpu(rtlib):
    assert rtlib.rt_device_count() > 0, "GPU tests need a device; the product has no CPU fallback"
    yield 0
    for v in _VOLUMES.values():
        v.close()
    for s in _SCENES.values():
        s.close()
    _VOLUMES.clear(), _SCENES.clear()


_SCENES, _DESCS, _ORACLES, _VOLUMES, _BAKED = {}, {}, {}, {}, {}


def desc(name):
    if name not in _DESCS:
        _DESCS[name] = scenes.get_scene(name)
    return _DESCS[name]


def grid_of(name):
    if GRIDS[name] is not None:
        return GRIDS[name]
    v = desc(name).world_triangles().reshape(-1, 3).astype(np.float64)
    lo, ext = v.min(0), v.max(0) - v.min(0)
    return tuple(lo + 0.2 * ext), (0.3 * ext[0], 0.6 * ext[1], 0.6 * ext[2]), (3, 2, 2)


def scene_of(name, gpu):
    if name not in _SCENES:
        _SCENES[name] = Scene(desc(name), device=gpu)
    return _SCENES[name]


def volume_of(name, gpu):
    """one volume per scene with room for MAX_DIRS directions, shared by the tests"""
    if name not in _VOLUMES:
        _VOLUMES[name] = ProbeVolume(scene_of(name, gpu), *grid_of(name), max_dirs=MAX_DIRS)
    return _VOLUMES[name]


def oracle_of(name, oracle):
    if name not in _ORACLES:
        _ORACLES[name] = oracle.OracleScene(desc(name))
    return _ORACLES[name]


def expected_bake(name, oracle, dirs, rr_start):
    """bake_model around the oracle, computed once per case and left unchanged"""
    key = (name, dirs, rr_start)
    if key not in _BAKED:
        v = _VOLUMES[name]  # (the wrapper holds the origin and the spacing as the fp32 values the library was given)
        sh, stats = bake_model(oracle_of(name, oracle).trace_paths, desc(name), v.origin, v.spacing, v.count, dirs, DEPTH, rr_start, SEED)
        sh.setflags(write=False)
        _BAKED[key] = (sh, stats)
    return _BAKED[key]


# ---- 1. entries ------------------------------------------------------------------------------------------------------------------------------
def assert_entries(v, dirs, seed):
    want = entries_model(v.origin, v.spacing, v.count, dirs, seed)
    got = v.entries(dirs, seed)
    for k in ("pos", "dir", "state"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    return want


@pytest.mark.parametrize("count", [(3, 2, 2), (3, 1, 2), (1, 1, 1)], ids=lambda c: "x".join(map(str, c)))
def test_entries_equal_the_model(gpu, count):
    v = ProbeVolume(scene_of("empty", gpu), (0.25, -1.0, 3.0), (0.7, 0.8, 1.3), count, max_dirs=37)
    want = assert_entries(v, 37, SEED)  # 444 entries at 3 x 2 x 2: seven waves, the last one part full
    assert len(want["state"]) == 37 * count[0] * count[1] * count[2]
    np.testing.assert_array_equal(want["pos"][::37], v.positions())
    assert_entries(v, 5, 0xFFFFFFFF)  # fewer directions than max_dirs
    v.close()


def test_entries_take_the_fallback_branch_at_the_state_the_search_found(gpu):
    s = fallback_state()
    assert s is not None
    v = ProbeVolume(scene_of("empty", gpu), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (3, 2, 2), max_dirs=37)
    want = assert_entries(v, 37, (s - 0x9E3779B9) & 0xFFFFFFFF)
    assert want["fallback"][0] and want["fallback"].sum() == 1
    v.close()


def test_entries_in_the_device_form_with_outputs_left_out(gpu):
    import torch
    v = ProbeVolume(scene_of("empty", gpu), (0.0, 0.0, 0.0), (1.0, 2.0, 3.0), (3, 2, 2), max_dirs=37)
    want = entries_model(v.origin, v.spacing, v.count, 37, SEED)
    n = 444
    st = torch.cuda.Stream(device=0)
    for mask in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        pos, d = (torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda") for _ in range(2))
        state = torch.full((n,), 0x55555555, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        v.entries_device(37, SEED, pos.data_ptr() * mask[0], d.data_ptr() * mask[1], state.data_ptr() * mask[2], stream=st.cuda_stream)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(pos.cpu().numpy(), want["pos"] if mask[0] else np.full((n, 3), 7.0, f32))
        np.testing.assert_array_equal(d.cpu().numpy(), want["dir"] if mask[1] else np.full((n, 3), 7.0, f32))
        np.testing.assert_array_equal(state.cpu().numpy().view(np.uint32), want["state"] if mask[2] else np.full(n, 0x55555555, np.uint32))
    with pytest.raises(abi.RtError) as e:
        v.entries_device(37, SEED)
    assert e.value.status == abi.RT_ERR_INVALID
    v.close()


# ---- 2. bake against the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rr_start", [0, 2])
@pytest.mark.parametrize("dirs", [37, 64])
@pytest.mark.parametrize("name", ["cornell", "tables", "empty"])
def test_a_bake_is_the_model_around_the_oracles_paths(gpu, oracle, name, dirs, rr_start):
    v = volume_of(name, gpu)
    want, stats = expected_bake(name, oracle, dirs, rr_start)
    sh, got = v.bake(dirs, DEPTH, rr_start, SEED)
    np.testing.assert_array_equal(sh, want)
    assert got == stats and stats["valid"] == stats["probes"] == 12 and stats["rays"] >= 12 * dirs
    np.testing.assert_array_equal(v.get_sh(), want)  # the table stays in the volume
    assert (sh[:, 0, 3] == 1).all() and (sh[:, 1:, 3] == 0).all() and (sh[:, 0, :3] > 0).any()
    if name != "empty":
        assert stats["rays"] > 12 * dirs


def test_a_probe_outside_the_contract_range_is_invalid_and_not_counted(gpu, oracle):
    sd = desc("cornell")
    v = ProbeVolume(scene_of("cornell", gpu), (0.0, 0.0, 0.0), (1000.0, 0.5, 0.5), (2, 2, 1), max_dirs=37)
    inside = contract_range_model(sd)(v.positions())
    np.testing.assert_array_equal(inside, [True, False, True, False])
    want, stats = bake_model(oracle_of("cornell", oracle).trace_paths, sd, v.origin, v.spacing, v.count, 37, DEPTH, 0, SEED)
    sh, got = v.bake(37, DEPTH, 0, SEED)
    np.testing.assert_array_equal(sh, want)
    assert got == stats and got["probes"] == 4 and got["valid"] == 2
    assert (sh[~inside].view(np.uint32) == 0).all() and (sh[inside, 0, 3] == 1).all()
    assert got["rays"] >= 2 * 37
    # sampling between a valid and an invalid probe gives the valid one's value
    p = np.array([[400.0, 0.1, 0.0]], f32)
    np.testing.assert_array_equal(v.sample(p, np.array([[0.0, 1.0, 0.0]], f32)), sample_model(v.origin, v.spacing, v.count, want, p, [[0.0, 1.0, 0.0]]))
    v.close()


def test_a_probe_inside_a_solid_is_valid_and_equals_the_model(gpu, oracle):
    sd = desc("cornell")
    v = ProbeVolume(scene_of("cornell", gpu), (-0.35, -0.4, -0.3), (1.0, 1.0, 1.0), (1, 1, 1), max_dirs=64)  # the centre of the metal box
    want, stats = bake_model(oracle_of("cornell", oracle).trace_paths, sd, v.origin, v.spacing, v.count, 64, DEPTH, 0, SEED)
    sh, got = v.bake(64, DEPTH, 0, SEED)
    np.testing.assert_array_equal(sh, want)
    assert got == stats and got["valid"] == 1
    v.close()


def test_the_device_form_on_a_stream_with_stats_equals_the_host_form(gpu, oracle):
    import torch
    v = volume_of("cornell", gpu)
    want, stats = expected_bake("cornell", oracle, 37, 2)
    st = torch.cuda.Stream(device=0)
    for want_sh, want_stats in ((True, True), (False, False)):
        sh = torch.full((12, 9, 4), 7.0, dtype=torch.float32, device="cuda")
        words = torch.full((2,), 0x5555555555555555, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        v.bake_device(37, DEPTH, 2, SEED, d_sh=sh.data_ptr() if want_sh else 0, d_stats=words.data_ptr() if want_stats else 0, stream=st.cuda_stream)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(v.get_sh(), want)
        w = words.cpu().numpy()
        if want_sh:
            np.testing.assert_array_equal(sh.cpu().numpy(), want)
            assert {"probes": int(w.view(np.uint32)[0]), "valid": int(w.view(np.uint32)[1]), "rays": int(w.view(np.uint64)[1])} == stats
        else:
            assert (sh.cpu().numpy() == 7.0).all() and (w.view(np.uint32) == 0x55555555).all()


def test_bake_and_sample_refusals_that_need_a_volume(gpu):
    v = ProbeVolume(scene_of("empty", gpu), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 2, 2), max_dirs=8)
    pts = np.zeros((3, 3), f32)
    for call in (lambda: v.sample(pts, pts), lambda: v.get_sh()):
        with pytest.raises(abi.RtError) as e:
            call()
        assert e.value.status == abi.RT_ERR_INVALID and "no table" in str(e.value)
    for args, word in (((0, 5), "dirs"), ((9, 5), "max_dirs"), ((8, 0), "max_depth"), ((9, 0), "max_dirs")):
        with pytest.raises(abi.RtError) as e:
            v.bake(*args)
        assert e.value.status == abi.RT_ERR_INVALID and word in str(e.value), (args, str(e.value))
        with pytest.raises(abi.RtError) as e:
            v.bake_device(*args)
        assert e.value.status == abi.RT_ERR_INVALID
    with pytest.raises(abi.RtError):
        v.entries(9, 0)
    p = abi.rt_probe_bake_params(8, 5, 0, 1)
    assert v._lib.rt_probe_volume_entries(v.h, C.byref(p), None, None, None) == abi.RT_ERR_INVALID
    assert v._lib.rt_probe_volume_set_sh(v.h, None) == abi.RT_ERR_INVALID
    assert v._lib.rt_probe_volume_bake(v.h, C.byref(p), None, None) == abi.RT_OK  # both outputs may be left out
    assert v._lib.rt_probe_volume_sample(v.h, 3, abi.fptr(pts), None, abi.fptr(pts)) == abi.RT_ERR_INVALID
    assert v._lib.rt_probe_volume_sample(v.h, 0, None, None, None) == abi.RT_OK  # n == 0: nothing launched
    for bad in ((pts[:, :2], pts[:, :2]), (pts, pts[:2]), (pts.reshape(-1), pts.reshape(-1)), (pts.astype(np.int32), pts)):
        with pytest.raises(ValueError):
            v.sample(*bad)
    for bad in (np.zeros((8, 9, 3), f32), np.zeros((7, 9, 4), f32), np.zeros((8, 9, 4), np.float64)):
        with pytest.raises(ValueError):
            v.set_sh(bad)
    assert v.bake(8, 5)[1]["valid"] == 8  # max_dirs itself is allowed
    v.close()


# ---- 3. sample ----------------------------------------------------------------------------------------------------------------------------------
def sample_points(origin, spacing, count, n, seed):
    """n points and normals: every probe position, points on cell faces (one coordinate on a probe plane), a shell outside the volume on
    every side (each axis below, inside and above), then points uniform in the volume grown by one spacing; unit normals, the six axis
    normals first."""
    g = np.random.default_rng(seed)
    origin, spacing = np.asarray(origin, f32), np.asarray(spacing, f32)
    P = probe_positions(origin, spacing, count)
    top = origin + spacing * (np.asarray(count, f32) - 1)
    faces = P[g.integers(0, len(P), 24)].copy()
    ax = g.integers(0, 3, 24)
    keep = np.arange(3)[None, :] == ax[:, None]
    faces = np.where(keep, faces, faces + (g.uniform(0.05, 0.95, size=(24, 3)) * spacing).astype(f32))
    shell = np.stack(np.meshgrid(*[[origin[a] - 2.5 * spacing[a], 0.5 * (origin[a] + top[a]), top[a] + 2.5 * spacing[a]] for a in range(3)],
                                 indexing="ij"), -1).reshape(-1, 3).astype(f32)
    fixed = np.concatenate([P, faces, shell])
    rest = g.uniform(origin - spacing, top + spacing, size=(max(n - len(fixed), 0), 3)).astype(f32)
    pos = np.concatenate([fixed, rest])[:n]
    nrm = g.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(f32)
    nrm[:6] = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f32)[:min(n, 6)]
    return np.ascontiguousarray(pos), np.ascontiguousarray(nrm)


def synthetic_table(probes, seed, invalid):
    g = np.random.default_rng(seed)
    sh = np.zeros((probes, 9, 4), f32)
    sh[:, :, :3] = g.normal(size=(probes, 9, 3)) * 0.3
    sh[:, 0, :3] = g.uniform(0.5, 3.0, size=(probes, 3))
    sh[:, 0, 3] = 1.0
    sh[list(invalid)] = 0.0
    return sh


@pytest.mark.parametrize("n", [1000, 65])
def test_samples_of_a_baked_table_equal_the_model(gpu, oracle, n):
    v = volume_of("cornell", gpu)
    want, _ = expected_bake("cornell", oracle, 64, 0)
    v.set_sh(np.array(want))
    pos, nrm = sample_points(v.origin, v.spacing, v.count, n, 3)
    out = v.sample(pos, nrm)
    np.testing.assert_array_equal(out, sample_model(v.origin, v.spacing, v.count, want, pos, nrm))
    assert (out > 0).any() and np.isfinite(out).all()


@pytest.mark.parametrize("count,invalid", [((3, 2, 2), (1, 6)), ((4, 3, 5), (0, 7, 8, 30, 59)), ((1, 1, 1), ()), ((1, 4, 1), (2,)), ((2, 1, 3), (5,)),
                                           ((2, 2, 2), tuple(range(8)))], ids=lambda c: "-".join(map(str, c)) or "none")
def test_samples_of_synthetic_tables_with_invalid_probes_equal_the_model(gpu, count, invalid):
    probes = count[0] * count[1] * count[2]
    v = ProbeVolume(scene_of("empty", gpu), (-1.0, 0.5, 2.0), (0.5, 1.25, 0.25), count, max_dirs=1)  # (positions exact in fp32)
    sh = synthetic_table(probes, 5, invalid)
    v.set_sh(sh)
    np.testing.assert_array_equal(v.get_sh(), sh)
    pos, nrm = sample_points(v.origin, v.spacing, count, 1000, 4)
    out = v.sample(pos, nrm)
    np.testing.assert_array_equal(out, sample_model(v.origin, v.spacing, count, sh, pos, nrm))
    if len(invalid) == probes:
        assert (out == 0).all()  # every corner invalid: W == 0
    elif invalid:
        on_invalid = v.sample(probe_positions(v.origin, v.spacing, count)[list(invalid)], np.tile(np.array([[0, 1, 0]], f32), (len(invalid), 1)))
        assert (on_invalid == 0).all()  # on an invalid probe the whole weight is its own
    v.close()


def test_points_and_normals_that_are_not_finite_give_nans(gpu):
    v = ProbeVolume(scene_of("empty", gpu), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 2, 2), max_dirs=1)
    sh = synthetic_table(8, 6, ())
    v.set_sh(sh)
    nan, inf = np.nan, np.inf
    pos = np.array([[nan, 0, 0], [0, inf, 0], [0, 0, -inf], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [3e38, -3e38, 0.5]], f32)
    nrm = np.array([[0, 1, 0], [0, 1, 0], [0, 1, 0], [nan, 0, 0], [0, 0, inf], [0, 1, 0], [0, 1, 0]], f32)
    out = v.sample(pos, nrm)
    assert np.isnan(out[:5]).all() and np.isfinite(out[5:]).all()
    np.testing.assert_array_equal(out, sample_model(v.origin, v.spacing, v.count, sh, pos, nrm))
    v.close()


def test_the_host_form_stages_more_points_than_one_piece(gpu):
    v = ProbeVolume(scene_of("empty", gpu), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (3, 3, 3), max_dirs=1)
    sh = synthetic_table(27, 8, (13,))
    v.set_sh(sh)
    pos, nrm = sample_points(v.origin, v.spacing, v.count, 65536 + 65, 9)
    np.testing.assert_array_equal(v.sample(pos, nrm), sample_model(v.origin, v.spacing, v.count, sh, pos, nrm))
    v.close()


def test_shade_vertices_from_volume_is_a_sample_at_the_mesh_corners(gpu, oracle):
    v = volume_of("cornell", gpu)
    want, _ = expected_bake("cornell", oracle, 64, 0)
    v.set_sh(np.array(want))
    cube = scenes.get_scene("cube")
    pos, nrm = bake.vertex_points(cube)
    out = bake.shade_vertices_from_volume(v, cube)
    assert out.shape == (cube.n_triangles, 3, 3)
    np.testing.assert_array_equal(out.reshape(-1, 3), sample_model(v.origin, v.spacing, v.count, want, pos.reshape(-1, 3), nrm.reshape(-1, 3)))


# ---- 4. ordering ----------------------------------------------------------------------------------------------------------------------------------
def test_a_sample_on_another_stream_waits_for_the_bake(gpu, oracle):
    import torch
    v = volume_of("cornell", gpu)
    want, _ = expected_bake("cornell", oracle, 64, 2)
    v.set_sh(synthetic_table(12, 1, ()))  # what a sample that did not wait would read
    pos, nrm = sample_points(v.origin, v.spacing, v.count, 1000, 5)
    d_pos, d_nrm = torch.from_numpy(pos).cuda(), torch.from_numpy(nrm).cuda()
    out = torch.full((1000, 3), 7.0, dtype=torch.float32, device="cuda")
    sa, sb = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    v.bake_device(64, DEPTH, 2, SEED, stream=sa.cuda_stream)
    v.sample_device(1000, d_pos.data_ptr(), d_nrm.data_ptr(), out.data_ptr(), stream=sb.cuda_stream)  # no host synchronisation in between
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), sample_model(v.origin, v.spacing, v.count, want, pos, nrm))


def test_a_bake_after_an_update_sees_the_moved_scene(gpu):
    from test_scene_update import spin_about_centre
    sd = desc("cornell")
    s = Scene(sd, device=gpu, updatable=True)
    v = ProbeVolume(s, *GRIDS["cornell"], max_dirs=37)
    before, _ = v.bake(37, DEPTH, 0, SEED)
    s.update(instances=spin_about_centre(sd, 25.0))
    after, stats = v.bake(37, DEPTH, 0, SEED)
    fresh = Scene(s.desc, device=gpu)
    v2 = ProbeVolume(fresh, *GRIDS["cornell"], max_dirs=37)
    moved, stats2 = v2.bake(37, DEPTH, 0, SEED)
    np.testing.assert_array_equal(after, moved)
    assert stats == stats2 and not np.array_equal(after, before)
    v2.close(), v.close(), fresh.close(), s.close()
