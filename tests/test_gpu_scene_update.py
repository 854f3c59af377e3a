"""Dynamic scenes on the MI355X: after rt_scene_update a scene renders, intersects and reports exactly what rt_scene_create of the updated
description (D') does — every renderer, schedule and tile split — and the device refit gives the tree and tables the host refit gives."""
import ctypes as C

import numpy as np
import pytest

from rtamd import abi, scenes
from rtamd.renderer import Camera, MegakernelRenderer, Scene, TileComm, WavefrontRenderer, assemble_tiles
from test_scene_update import (_tables_equal, _tree_equal, chain_scene, model_node_words, rays, same_bits, spin_about_centre,
                               update_sequence)

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H, DEPTH, SPP = 48, 32, 5, 4

CONFIGS = {
    "megakernel": (MegakernelRenderer, {}),
    "megakernel_slices": (MegakernelRenderer, dict(pixel_slices=4)),
    "wavefront": (WavefrontRenderer, {}),
    "wavefront_slices": (WavefrontRenderer, dict(pixel_slices=4)),
    "wavefront_per_bounce": (WavefrontRenderer, dict(finish_depth=abi.RT_SCHED_ALL_BOUNCES)),
    "wavefront_fused": (WavefrontRenderer, dict(finish_depth=abi.RT_SCHED_ALL_BOUNCES, fused_bounce=True)),
    "wavefront_graph": (WavefrontRenderer, dict(hip_graph=True)),
}


def frame_of(cls, sched, scene, cam, spp=SPP):
    r = cls(scene, (W, H), DEPTH, spp)
    if sched:
        r.set_schedule(**sched)
    fr = r.render_frame(cam)
    r.close()
    return fr


def assert_same_frame(a, b):
    assert a.rays == b.rays
    np.testing.assert_array_equal(a.rgba_f32, b.rgba_f32)
    np.testing.assert_array_equal(a.rgba_u8, b.rgba_u8)


def gpu_updates(sd):
    """Three successive updates: a rotation of every instance, a mirror and a translation, an edit of positions and normals."""
    seq = update_sequence(sd)
    return [seq[0], seq[1], seq[3]]


@pytest.mark.parametrize("config", list(CONFIGS))
def test_frames_after_updates_equal_a_fresh_scene(devlib, scene_cache, config):
    cls, sched = CONFIGS[config]
    sd = scene_cache("cornell")
    cam = Camera.for_scene(sd, (W, H))
    s = Scene(sd, 0, abi.RT_BVH_SAH, lib=devlib, updatable=True)
    r = cls(s, (W, H), DEPTH, SPP)
    if sched:
        r.set_schedule(**sched)
    assert_same_frame(r.render_frame(cam), frame_of(cls, sched, Scene(sd, 0, abi.RT_BVH_SAH, lib=devlib), cam))
    for k, u in enumerate(gpu_updates(sd)):
        st = s.update(**u)
        assert st.launches >= 3 and st.refit_nodes == s.info().n_nodes and st.device_ms > 0.0
        fr = r.render_frame(cam)
        fresh = Scene(s.desc, 0, abi.RT_BVH_SAH, lib=devlib)
        assert_same_frame(fr, frame_of(cls, sched, fresh, cam))
        fresh.close()
        if sched.get("hip_graph"):
            n = C.c_uint32()
            abi.check(devlib.rt_dev_renderer_graph_captures(r.h, C.byref(n)), devlib)
            assert n.value == k + 2  # the graph of the first frame, then one more per update
            r.render_frame(cam)
            abi.check(devlib.rt_dev_renderer_graph_captures(r.h, C.byref(n)), devlib)
            assert n.value == k + 2  # (and replayed while the scene stays as it is)
    r.close()
    s.close()


@pytest.mark.parametrize("bvh", [abi.RT_BVH_LBVH, abi.RT_BVH_LBVH_GPU])
def test_frames_after_updates_of_other_builders(devlib, scene_cache, bvh):
    sd = scene_cache("atrium", detail=1)
    cam = Camera.for_scene(sd, (W, H))
    s = Scene(sd, 0, bvh, lib=devlib, updatable=True)
    r = WavefrontRenderer(s, (W, H), DEPTH, SPP)
    for u in gpu_updates(sd):
        s.update(**u)
        fresh = Scene(s.desc, 0, bvh, lib=devlib)
        assert_same_frame(r.render_frame(cam), frame_of(WavefrontRenderer, {}, fresh, cam))
        fresh.close()
    r.close()
    s.close()


def test_two_strip_split_gathers_the_updated_frame(scene_cache):
    sd = scene_cache("cornell")
    cam = Camera.for_scene(sd, (W, H))
    s = Scene(sd, 0, abi.RT_BVH_SAH, updatable=True)
    comm = TileComm((0, 0))
    rs = []
    for k in range(2):
        r = WavefrontRenderer(s, (W, H), DEPTH, SPP)
        r.set_tile(k, 2, 8)
        rs.append(r)
    for u in gpu_updates(sd):
        s.update(**u)
        fresh = Scene(s.desc, 0, abi.RT_BVH_SAH)
        exp = frame_of(WavefrontRenderer, {}, fresh, cam)
        f, b, rays_ = comm.render_and_gather(rs, cam)
        assert rays_ == exp.rays
        np.testing.assert_array_equal(f, exp.rgba_f32)
        np.testing.assert_array_equal(b, exp.rgba_u8)
        parts = [r.render_frame(cam) for r in rs]
        np.testing.assert_array_equal(assemble_tiles([p.rgba_f32 for p in parts], H, 2, 8), exp.rgba_f32)
        fresh.close()
    for r in rs:
        r.close()
    comm.close()
    s.close()


@pytest.mark.parametrize("bvh", [abi.RT_BVH_SAH, abi.RT_BVH_LBVH, abi.RT_BVH_LBVH_GPU])
def test_intersect_batch_after_updates(scene_cache, bvh):
    sd = scene_cache("atrium", detail=1)
    s = Scene(sd, 0, bvh, updatable=True)
    for u in update_sequence(sd):
        s.update(**u)
        org, d = rays(s.desc, 4000, seed=11)
        fresh = Scene(s.desc, 0, bvh)
        for a, b in zip(s.intersect(org, d), fresh.intersect(org, d)):
            assert same_bits(a, b)
        fresh.close()
        info, finfo = s.info(), Scene(s.desc, -1, abi.RT_BVH_SAH).info()
        assert list(info.bounds_lo) == list(finfo.bounds_lo) and list(info.bounds_hi) == list(finfo.bounds_hi)
    s.close()


def test_updated_scene_matches_the_oracle(oracle, scene_cache):
    sd = scene_cache("cornell")
    s = Scene(sd, 0, abi.RT_BVH_SAH, updatable=True)
    for u in gpu_updates(sd):
        s.update(**u)
    osc = oracle.OracleScene(s.desc)
    ocam = oracle.camera(W, H, sd.camera.position, sd.camera.direction, sd.camera.focal_length)
    for cls, kind in ((MegakernelRenderer, abi.RT_RENDERER_MEGAKERNEL), (WavefrontRenderer, abi.RT_RENDERER_WAVEFRONT)):
        fr = frame_of(cls, {}, s, Camera.for_scene(sd, (W, H)), spp=2)
        f, b, n = osc.render(ocam, kind, DEPTH, 2, use_bvh=False)
        assert fr.rays == n
        np.testing.assert_array_equal(fr.rgba_f32, f)
        np.testing.assert_array_equal(fr.rgba_u8, b)
    s.close()


@pytest.mark.parametrize("bvh", [abi.RT_BVH_SAH, abi.RT_BVH_LBVH])
@pytest.mark.parametrize("name", ["atrium", "tables", "atrium_tilted"])
def test_device_update_equals_host_update(devlib, scene_cache, name, bvh):
    sd = scene_cache(name, detail=1) if name != "tables" else scene_cache("tables", n_mats=25, n_rows=6)
    dev = Scene(sd, 0, bvh, lib=devlib, updatable=True)
    host = Scene(sd, -1, bvh, lib=devlib, updatable=True)
    for u in update_sequence(sd):
        dev.update(**u)
        host.update(**u)
        _tree_equal(dev.tree(), host.tree())
        _tables_equal(dev.shading_tables(), host.shading_tables(), lds=False)
        fresh = Scene(dev.desc, 0, bvh, lib=devlib)
        _tables_equal(dev.shading_tables(), fresh.shading_tables())  # (lds_nm / lds_mats: what a device scene stages)
        fresh.close()
        dev.check_bvh()
        assert dev.info().sah_cost == pytest.approx(host.info().sah_cost, rel=1e-12)
    dev.close()
    host.close()


def test_device_built_lbvh_is_refit_to_the_model(devlib, scene_cache):
    """RT_BVH_LBVH_GPU (no host-only counterpart): after every update each node's words 0..11 are the quantised padded exact child boxes of
    the new world vertices, and vertices / bounds / pad are those of a fresh build."""
    for sd in (scene_cache("atrium", detail=1), chain_scene()):
        s = Scene(sd, 0, abi.RT_BVH_LBVH_GPU, lib=devlib, updatable=True)
        built = s.tree()
        for u in update_sequence(sd):
            s.update(**u)
            tree = s.tree()
            assert same_bits(tree["nodes"][:, 12:], built["nodes"][:, 12:]) and same_bits(tree["global_index"], built["global_index"])
            words, live = model_node_words(devlib, tree)
            assert same_bits(tree["nodes"][live, :12], words[live])
            ftree = Scene(s.desc, -1, abi.RT_BVH_SAH, lib=devlib).tree()
            for k in ("wverts", "pad", "bounds_lo", "bounds_hi"):
                assert same_bits(tree[k], ftree[k]), k
            s.check_bvh()
        s.close()


def test_refused_update_leaves_the_frame(devlib, scene_cache):
    sd = scene_cache("cornell")
    cam = Camera.for_scene(sd, (W, H))
    s = Scene(sd, 0, abi.RT_BVH_SAH, lib=devlib, updatable=True)
    s.update(**update_sequence(sd)[0])
    r = MegakernelRenderer(s, (W, H), DEPTH, SPP)
    before, tree = r.render_frame(cam), s.tree()
    xf = np.array(s.desc.transforms, f32, copy=True)
    xf[0] = scenes.mat4_mul(scenes.mat4_scale((3.0e38, 1.0, 1.0)), xf[0])
    xf[1] = scenes.mat4_mul(scenes.mat4_scale((-3.0e38, 1.0, 1.0)), xf[1])
    with pytest.raises(abi.RtError) as ei:
        s.update(instances=(xf, s.desc.normal_mats))
    assert ei.value.status == abi.RT_ERR_INVALID
    assert_same_frame(r.render_frame(cam), before)
    _tree_equal(s.tree(), tree)
    r.close()
    s.close()


def test_update_waits_for_frames_in_flight(scene_cache):
    sd = scene_cache("cornell")
    cam = Camera.for_scene(sd, (W, H))
    s = Scene(sd, 0, abi.RT_BVH_SAH, updatable=True)
    r = WavefrontRenderer(s, (W, H), DEPTH, SPP)
    u = update_sequence(sd)[0]
    r.begin_frame(cam, abi.load_library().rt_renderer_tile_f32(r.h), abi.load_library().rt_renderer_tile_u8(r.h))
    with pytest.raises(abi.RtError) as ei:
        s.update(**u)
    assert ei.value.status == abi.RT_ERR_INVALID and "in flight" in str(ei.value)
    r.end_frame()
    s.update(**u)
    fresh = Scene(s.desc, 0, abi.RT_BVH_SAH)
    assert_same_frame(r.render_frame(cam), frame_of(WavefrontRenderer, {}, fresh, cam))
    r.close()
    # a renderer destroyed with its frame in flight releases the scene too
    r2 = WavefrontRenderer(s, (W, H), DEPTH, SPP)
    r2.begin_frame(cam, abi.load_library().rt_renderer_tile_f32(r2.h), 0)
    r2.close()
    s.update(**update_sequence(sd)[1])
    fresh.close()
    s.close()


@pytest.mark.parametrize("cls", [MegakernelRenderer, WavefrontRenderer])
def test_progressive_state_ends_with_the_update(scene_cache, cls):
    sd = scene_cache("cornell")
    cam = Camera.for_scene(sd, (W, H))
    s = Scene(sd, 0, abi.RT_BVH_SAH, updatable=True)
    r = cls(s, (W, H), DEPTH, 2)
    r.set_progressive(True)
    r.render_frame(cam)
    r.continue_frame(1)
    assert r.accumulated_samples == 3
    xf, nm = spin_about_centre(sd, 20.0)
    s.update(instances=(xf, nm))
    assert r.accumulated_samples == 0
    with pytest.raises(abi.RtError) as ei:
        r.continue_frame(1)
    assert ei.value.status == abi.RT_ERR_INVALID
    with pytest.raises(abi.RtError):
        r.continue_blocks(1, [0])
    first = r.render_frame(cam)
    assert r.accumulated_samples == 2
    cont = r.continue_frame(3)
    fresh = Scene(s.desc, 0, abi.RT_BVH_SAH)
    exp = frame_of(cls, {}, fresh, cam, spp=5)
    assert first.rays + cont.rays == exp.rays
    np.testing.assert_array_equal(cont.rgba_f32, exp.rgba_f32)
    np.testing.assert_array_equal(cont.rgba_u8, exp.rgba_u8)
    fresh.close()
    r.close()
    s.close()
