"""The baked-lighting kernels on the GPU (csrc/rt_probe_volume.hip, csrc/rt_reflection.hip, csrc/rt_lightmap.hip) against the float64
light-transport integrals of tests/bake_maths.py: the checks of tests/test_bake_maths.py with the device's results in the numpy models'
place and the same bounds. Nothing on the expected side is a model of the header's arithmetic: k_pv_sample against the cosine-weighted
hemisphere integral, k_pv_entries + the path query + k_pv_project at max_depth = 1 against the solid-angle integrals of the patches seen from
each probe, k_rf_entries + the path query + k_rf_resolve + k_rf_sample against the coverage of rectangles placed in world space, k_lm_owner +
k_lm_texels against float64 barycentric geometry. The inputs (tables, points, scenes, UV sets) are those of tests/test_bake_maths.py."""
import numpy as np
import pytest

import bake_maths as bm
from rtamd import scenes
from rtamd.renderer import Lightmap, ProbeVolume, ReflectionProbes, Scene
from test_bake_maths import (COUNTS, GRID, LIGHTMAP_CASES, OFF_CENTRE, RECTS, SCENES, SEED, SPT, lightmap_case, patch_desc, sh_points, sh_table)

pytestmark = pytest.mark.gpu
f32 = np.float32
_SCENES = {}


@pytest.fixture(scope="module")
def gpu(rtlib):
    assert rtlib.rt_device_count() > 0, "GPU tests need a device; the product has no CPU fallback"
    yield 0
    for v in _VOLUMES.values():
        v.close()
    for s in _SCENES.values():
        s.close()
    _VOLUMES.clear(), _SCENES.clear()


def scene_of(key, sd, gpu):
    if key not in _SCENES:
        _SCENES[key] = Scene(sd, device=gpu)
    return _SCENES[key]


def empty_scene(gpu):
    return scene_of("empty", scenes.get_scene("empty"), gpu)


def on_device(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


# ---- k_pv_sample -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 1000])
@pytest.mark.parametrize("count,invalid", COUNTS, ids=lambda c: "-".join(map(str, c)) or "none")
def test_samples_are_the_cosine_weighted_integral_of_the_interpolated_radiance(gpu, count, invalid, n):
    import torch
    probes = count[0] * count[1] * count[2]
    v = ProbeVolume(empty_scene(gpu), GRID[0], GRID[1], count, max_dirs=1)
    pos, nrm = sh_points(count, n, 4)
    st = torch.cuda.Stream(device=0)
    for negative in (False, True):
        sh = sh_table(probes, 5, invalid, negative)
        v.set_sh(sh)
        host = v.sample(pos, nrm)
        ref, dark = bm.check_sh_sample(host, v.origin, v.spacing, count, sh, pos, nrm, "sh sample, device")
        assert (dark.any() and (ref > 0).any()) if negative else (ref >= 0).all()
        d_pos, d_nrm = on_device(pos, nrm)
        out = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        v.sample_device(n, d_pos.data_ptr(), d_nrm.data_ptr(), out.data_ptr(), stream=st.cuda_stream)
        torch.cuda.synchronize()
        bm.check_sh_sample(out.cpu().numpy(), v.origin, v.spacing, count, sh, pos, nrm, "sh sample, device form")
    v.close()


# ---- k_pv_entries + the path query + k_pv_project ---------------------------------------------------------------------------------------------
MAX_DIRS = 65536  # kMaxDirs
_VOLUMES = {}


def volume_of(key, gpu):
    """one volume per (scene, grid), with room for MAX_DIRS directions, shared by the two direction counts"""
    if key not in _VOLUMES:
        name, origin, spacing, count = key
        _VOLUMES[key] = ProbeVolume(scene_of(name, patch_desc(name), gpu), origin, spacing, count, max_dirs=MAX_DIRS)
    return _VOLUMES[key]


ONE = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1, 1, 1))
EIGHT = ((-0.3, -0.25, -0.2), (0.55, 0.45, 0.5), (2, 2, 2))  # eight different points inside the cube: 72 (probe, k) lanes


@pytest.mark.parametrize("dirs", [4096, MAX_DIRS])
@pytest.mark.parametrize("name,grid", [("lid", ONE), ("patches", ONE), ("patches", EIGHT)], ids=["lid-1", "patches-1", "patches-8"])
def test_a_depth_1_bake_is_the_sky_minus_the_patches_seen_from_each_probe(gpu, name, grid, dirs):
    v = volume_of((name,) + grid, gpu)
    sh, stats = v.bake(dirs, 1, 0, SEED)
    eyes = v.positions()
    assert len(eyes) == grid[2][0] * grid[2][1] * grid[2][2] and (np.abs(eyes) < 0.5).all()
    bm.check_sh_bake(sh, stats, SCENES[name], eyes, np.ones(len(eyes), bool), dirs, patch_desc(name).sky, "sh bake, device")
    np.testing.assert_array_equal(v.get_sh(), sh)
    if dirs == MAX_DIRS:  # the last use of the volume
        _VOLUMES.pop((name,) + grid).close()


def test_a_probe_outside_the_contract_range_stays_invalid_and_zero_beside_a_valid_one(gpu):
    v = ProbeVolume(scene_of("patches", patch_desc("patches"), gpu), OFF_CENTRE, (1000.0, 1.0, 1.0), (2, 1, 1), max_dirs=4096)
    sh, stats = v.bake(4096, 1, 0, SEED)
    bm.check_sh_bake(sh, stats, RECTS, v.positions(), [True, False], 4096, patch_desc("patches").sky, "sh bake, device")
    v.close()


# ---- k_rf_entries + the path query + k_rf_resolve + k_rf_sample ---------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [16, 32])
def test_a_depth_1_capture_shows_the_patches_where_world_space_has_them(gpu, size):
    import torch
    sd = patch_desc("patches")
    centres = np.array([OFF_CENTRE, (1000.0, 0.0, 0.0), (0.0, 0.0, 0.0)], f32)  # off centre, outside the contract range, the origin
    r = ReflectionProbes(scene_of("patches", sd, gpu), centres, size, 1, SPT)
    chain, stats = r.bake(SPT, 1, 0, SEED)
    assert stats == {"probes": 3, "valid": 2, "rays": 2 * 6 * size * size * SPT}
    lv = r.level(chain, 0)
    assert (lv[1].view(np.uint32) == 0).all()
    n_open, n_blocked, n_partial = bm.check_cube_level0(lv[2], RECTS, SPT, sd.sky, "cube level 0, device")
    assert n_open + n_blocked + n_partial == 6 * size * size and n_blocked >= 6 * 4 and n_partial >= 6 * 8
    bm.check_cube_classes(lv[0], *bm.texel_classes(size, RECTS, centres[0]), SPT, sd.sky, "cube level 0 off centre, device")
    # the lookups: the host form, then the device form on a stream
    dirs, blocked = bm.cube_sample_cases(size, RECTS)
    n = len(dirs)
    idx, d32, lod = np.full(n, 2, np.uint32), np.ascontiguousarray(dirs, f32), np.zeros(n, f32)
    bm.check_cube_samples(r.sample(idx, d32, lod), blocked, SPT, sd.sky, "cube sample, device")
    d_idx, d_dir, d_lod = on_device(idx.view(np.int32), d32, lod)
    out = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    r.sample_device(n, d_idx.data_ptr(), 0, d_dir.data_ptr(), d_lod.data_ptr(), out.data_ptr(), stream=st.cuda_stream)
    torch.cuda.synchronize()
    bm.check_cube_samples(out.cpu().numpy(), blocked, SPT, sd.sky, "cube sample, device form")
    r.close()


# ---- k_lm_owner + k_lm_texels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,W,H", LIGHTMAP_CASES, ids=lambda v: str(v))
def test_every_texel_lies_on_the_surface_point_under_its_centre(gpu, name, W, H):
    sd, uv = lightmap_case(name, W, H)
    lm = Lightmap(scene_of((name, len(uv)), sd, gpu), uv, W, H)
    got = lm.texels()
    lm.close()
    bm.check_lightmap(got["tri"], got["pos"], got["normal"], sd, uv, W, H, f"lightmap {name} {W}x{H}, device")
