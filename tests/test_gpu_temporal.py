"""GPU tests of the temporal stage: the per-frame seed salt (rt_renderer_set_frame_seed), the motion guide (rt_scene_gbuffer_motion[_device]) and
the accumulator (rt_temporal_accumulate[_device]), the last two pinned bit for bit to the numpy float32 models of tests/test_temporal.py; the
stage's quality against a 1024-spp frame and the CLI's --temporal."""
import ctypes as C
import importlib.util
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rtamd import abi
from rtamd.renderer import (Camera, Denoiser, MegakernelRenderer, Scene, TemporalAccumulator, WavefrontRenderer, assemble_tiles,
                            TEMPORAL_COS_NORMAL, TEMPORAL_MAX_HISTORY, temporal_params)
from test_scene_update import spin_about_centre
from test_temporal import motion_model, temporal_model, world_vertices_f32

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden"
EXE = REPO / "sycl-ray-tracer_amd" / "host" / "build" / "raytracer"
f32 = np.float32
INF = float("inf")
KINDS = [MegakernelRenderer, WavefrontRenderer]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_frame(a, b):
    return same_bits(a.rgba_f32, b.rgba_f32) and same_bits(a.rgba_u8, b.rgba_u8) and a.rays == b.rays


def camera_rays(cam):
    w, h = int(cam.width), int(cam.height)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    xs, ys = xs.reshape(-1).astype(f32), ys.reshape(-1).astype(f32)
    p00, du, dv, ce = (np.array(list(v), f32) for v in (cam.pixel00, cam.delta_u, cam.delta_v, cam.center))
    d = ((p00[None, :] + xs[:, None] * du[None, :]) + ys[:, None] * dv[None, :]) - ce[None, :]
    return np.broadcast_to(ce, d.shape).copy(), d


def linear_rmse(a, ref):
    """RMSE in linear radiance of two frames (rgb = sqrt(mean))."""
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) ** 2 - ref[..., :3].astype(np.float64) ** 2) ** 2)))


# ---- the seed salt -----------------------------------------------------------------------------------------------------------------------
def _golden_cases():
    spec = importlib.util.spec_from_file_location("make_golden", GOLDEN / "make_golden.py")
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg.CASES


# (every fixture of make_golden.py; host_walks.npz is make_host_walks.py's, held by tests/test_host_walks.py)
@pytest.mark.parametrize("case", sorted(p.stem for p in GOLDEN.glob("*.npz") if p.stem != "host_walks"))
def test_salt_zero_is_the_golden_frame_and_a_salt_is_reproducible(rtlib, scene_cache, case):
    name, kw, w, h, spp, depth = _golden_cases()[case]
    g = np.load(GOLDEN / f"{case}.npz")
    sd = scene_cache(name, **kw)
    s = Scene(sd, device=0)
    cam = Camera.for_scene(sd, (w, h))
    for cls, tag in ((MegakernelRenderer, "mega"), (WavefrontRenderer, "wave")):
        r = cls(s, (w, h), depth, spp)
        plain = r.render_frame(cam)  # no call at all
        assert same_bits(plain.rgba_f32, g[f"{tag}_f32"]) and same_bits(plain.rgba_u8, g[f"{tag}_u8"]) and plain.rays == int(g[f"{tag}_rays"])
        r.set_frame_seed(0)
        assert same_frame(r.render_frame(cam), plain), (case, tag)
        r.set_frame_seed(5)
        a = r.render_frame(cam)
        assert same_frame(r.render_frame(cam), a), (case, tag)      # the same salt twice
        r2 = cls(s, (w, h), depth, spp)
        r2.set_frame_seed(5)
        assert same_frame(r2.render_frame(cam), a), (case, tag)     # ... and in another renderer
        r.set_frame_seed(0xFFFFFFFF)
        b = r.render_frame(cam)
        assert not same_bits(a.rgba_f32, plain.rgba_f32) and not same_bits(a.rgba_f32, b.rgba_f32), (case, tag)  # two salts: frames differ
        r.set_frame_seed(0)
        assert same_frame(r.render_frame(cam), plain), (case, tag)  # back to the reference's seeds
        r.close(), r2.close()
    s.close()


@pytest.mark.parametrize("seed_mode", [abi.RT_SEED_WAVEFRONT, abi.RT_SEED_MEGAKERNEL])
def test_renderers_with_equal_seeds_stay_equal_under_a_salt(rtlib, scene_cache, seed_mode):
    """tests/test_gpu_parity.py: test_megakernel_equals_wavefront_with_equal_seeds, under a salt."""
    for name in ("triangle", "cube"):
        sd = scene_cache(name)
        s = Scene(sd, device=0)
        w, h = 200, 120
        cam = Camera.for_scene(sd, (w, h))
        a, b = MegakernelRenderer(s, (w, h), 10, 6, seed_mode), WavefrontRenderer(s, (w, h), 10, 6, seed_mode)
        a.set_frame_seed(77), b.set_frame_seed(77)
        assert same_frame(a.render_frame(cam), b.render_frame(cam)), name
        a.close(), b.close(), s.close()


def test_frame_seed_is_refused_while_a_frame_is_in_flight(rtlib, scene_cache):
    sd = scene_cache("cornell")
    s = Scene(sd, device=0)
    cam = Camera.for_scene(sd, (64, 48))
    for cls in KINDS:
        r = cls(s, (64, 48), 6, 2)
        r.begin_frame(cam)
        with pytest.raises(abi.RtError) as e:
            r.set_frame_seed(3)
        assert e.value.status == abi.RT_ERR_INVALID
        r.end_frame()
        r.set_frame_seed(3)
        r.close()
    s.close()


def test_salted_frames_under_schedules_slices_tiles_and_graphs(rtlib, scene_cache):
    sd = scene_cache("cornell")
    s = Scene(sd, device=0)
    w, h, depth, spp, salt = 120, 93, 10, 8, 12345
    cam = Camera.for_scene(sd, (w, h))
    for cls in KINDS:
        r = cls(s, (w, h), depth, spp)
        r.set_frame_seed(salt)
        plain = r.render_frame(cam)
        r.set_frame_seed(salt + 1)
        other = r.render_frame(cam)
        assert not same_bits(plain.rgba_f32, other.rgba_f32)
        r.set_frame_seed(salt)
        scheds = [dict(pixel_slices=2), dict(pixel_slices=4), dict(pixel_slices=0)]
        if cls is WavefrontRenderer:
            scheds += [dict(samples_per_launch=1), dict(samples_per_launch=2, requeue=1), dict(finish_depth=abi.RT_SCHED_ALL_BOUNCES),
                       dict(finish_depth=abi.RT_SCHED_ALL_BOUNCES, fused_bounce=True), dict(finish_depth=2), dict(stream_lanes=2, samples_per_launch=1)]
        for sc in scheds:
            r.set_schedule(**sc)
            assert same_frame(r.render_frame(cam), plain), (cls.__name__, sc)
        if cls is WavefrontRenderer:  # a captured graph: replayed with its salt, re-captured when the salt changes
            for sc in (dict(hip_graph=True), dict(hip_graph=True, finish_depth=abi.RT_SCHED_ALL_BOUNCES)):
                r.set_schedule(**sc)
                r.set_frame_seed(salt)
                assert same_frame(r.render_frame(cam), plain) and same_frame(r.render_frame(cam), plain), sc
                r.set_frame_seed(salt + 1)
                assert same_frame(r.render_frame(cam), other), sc
                r.set_frame_seed(salt)
                assert same_frame(r.render_frame(cam), plain), sc
        r.set_schedule()
        for world in (2, 3):  # seeds are a function of global pixel coordinates: the tiles union to the frame
            parts, rays = [], 0
            for rank in range(world):
                r.set_tile(rank, world, 8)
                fr = r.render_frame(cam)
                parts.append(fr.rgba_f32)
                rays += fr.rays
            assert rays == plain.rays and same_bits(assemble_tiles(parts, h, world, 8), plain.rgba_f32), (cls.__name__, world)
        r.close()
    s.close()


@pytest.mark.parametrize("cls", KINDS)
def test_salted_progressive_chain(rtlib, scene_cache, cls):
    sd = scene_cache("cornell")
    s = Scene(sd, device=0)
    w, h, a, b, salt = 96, 64, 3, 5, 9
    cam = Camera.for_scene(sd, (w, h))
    whole = cls(s, (w, h), 10, a + b)
    whole.set_frame_seed(salt)
    want = whole.render_frame(cam)
    r = cls(s, (w, h), 10, a)
    r.set_progressive(True)
    r.set_frame_seed(salt)
    first = r.render_frame(cam)
    r.set_frame_seed(salt + 100)  # a continuation continues the chain it was started with
    more = r.continue_frame(b)
    assert same_bits(more.rgba_f32, want.rgba_f32) and same_bits(more.rgba_u8, want.rgba_u8) and first.rays + more.rays == want.rays
    nxt = r.render_frame(cam)  # the next FRAME starts with the new salt
    chk = cls(s, (w, h), 10, a)
    chk.set_frame_seed(salt + 100)
    assert same_frame(nxt, chk.render_frame(cam))
    whole.close(), r.close(), chk.close(), s.close()


def test_salted_frames_are_independent_samples(rtlib, scene_cache):
    """The property the salt exists for. The mean, in linear radiance, of 16 one-spp frames with salts 1 .. 16 against a 1024-spp frame: its
    RMSE must lie below that of ONE 4-spp frame. (Independent samples would give half of it, sigma / 4 against sigma / 2: the assertion leaves a
    factor 2 for the correlation of xorshift chains started at neighbouring words. Measured on the MI355X: DESIGN.md §15.)"""
    sd = scene_cache("atrium")
    w, h, depth = 320, 180, 10
    s = Scene(sd, device=0)
    cam = Camera.for_scene(sd, (w, h))
    ref = MegakernelRenderer(s, (w, h), depth, 1024).render_frame(cam, want_u8=False).rgba_f32
    four = MegakernelRenderer(s, (w, h), depth, 4).render_frame(cam, want_u8=False).rgba_f32
    one = MegakernelRenderer(s, (w, h), depth, 1)
    acc = np.zeros((h, w, 3), np.float64)
    for salt in range(1, 17):
        one.set_frame_seed(salt)
        acc += one.render_frame(cam, want_u8=False).rgba_f32[..., :3].astype(np.float64) ** 2
    mean16 = np.sqrt(acc / 16)
    one.set_frame_seed(0)
    plain = one.render_frame(cam, want_u8=False).rgba_f32
    for _ in range(3):  # with salt 0 throughout every frame is the same frame: the "mean" is the 1-spp frame itself
        assert same_bits(one.render_frame(cam, want_u8=False).rgba_f32, plain)
    e_mean, e_four, e_one = linear_rmse(mean16, ref), linear_rmse(four, ref), linear_rmse(plain, ref)
    print(f"\nindependence 320x180 atrium: RMSE mean of 16 salted 1-spp frames {e_mean:.6f}, one 4-spp frame {e_four:.6f}, one 1-spp frame {e_one:.6f}")
    assert e_mean < e_four, (e_mean, e_four, e_one)
    s.close()


# ---- the motion guide --------------------------------------------------------------------------------------------------------------------
def check_motion(scene, prev_world, cam):
    """gbuffer_motion == gbuffer + motion_model(previous world vertices), bit for bit; returns the four planes."""
    g = scene.gbuffer_motion(cam)
    plain = scene.gbuffer(cam)
    for k in plain:
        assert same_bits(g[k], plain[k]), k
    org, d = camera_rays(cam.c)
    t, u, v, tri = scene.intersect(org, d)
    m = motion_model(prev_world, u, v, tri, int(cam.c.width), int(cam.c.height))
    assert same_bits(g["prev_position"], m), np.argwhere(g["prev_position"].view(np.uint32) != m.view(np.uint32))[:4]
    return g


def vertex_edit(sd, seed=5):
    rng = np.random.default_rng(seed)
    return (np.asarray(sd.positions, f32) + rng.normal(scale=1e-2, size=np.asarray(sd.positions).shape).astype(f32)).astype(f32)


@pytest.mark.parametrize("bvh", [abi.RT_BVH_SAH, abi.RT_BVH_LBVH, abi.RT_BVH_LBVH_GPU])
@pytest.mark.parametrize("name", ["atrium", "atrium_tilted"])  # atrium_tilted: the SAH builder pre-splits its large triangles
def test_motion_guide_equals_the_model(rtlib, scene_cache, name, bvh):
    sd0 = scene_cache(name)
    s = Scene(sd0, device=0, bvh=bvh, updatable=True, keep_previous=True)
    if name == "atrium_tilted" and bvh == abi.RT_BVH_SAH:
        assert s.info().n_split_triangles > 0
    cam = Camera.for_scene(sd0, (160, 90))
    tol = 1e-4 * float(s.scale())
    w0 = world_vertices_f32(sd0)
    g0 = check_motion(s, w0, cam)  # before any update previous == current
    hit = np.isfinite(g0["position"][..., 3])
    assert hit.any() and (g0["prev_position"][hit][:, 3] == 1).all() and (g0["prev_position"][~hit] == 0).all()
    assert np.allclose(g0["prev_position"][hit][:, :3], g0["position"][hit][:, :3], rtol=0, atol=tol)
    s.update(instances=spin_about_centre(sd0, 4.0))
    sd1 = s.desc
    g1 = check_motion(s, w0, cam)  # after an instance spin: where the surface was
    moved = np.isfinite(g1["position"][..., 3])
    assert not np.allclose(g1["prev_position"][moved][:, :3], g1["position"][moved][:, :3], rtol=0, atol=tol)
    s.update(positions=vertex_edit(sd1))
    sd2 = s.desc
    check_motion(s, world_vertices_f32(sd1), cam)  # after a vertex update; previous is the state ONE update ago, not the original
    xf_bad = np.array(sd2.transforms, f32, copy=True)
    xf_bad[0, 12] = np.nan
    before = s.gbuffer_motion(cam)
    with pytest.raises(abi.RtError) as e:
        s.update(instances=(xf_bad, np.asarray(sd2.normal_mats, f32)))
    assert e.value.status == abi.RT_ERR_INVALID
    after = s.gbuffer_motion(cam)  # a refused update leaves the guide (and the scene) unchanged
    for k in before:
        assert same_bits(before[k], after[k]), k
    s.update(normals=np.asarray(sd2.normals, f32))  # an update that moves nothing: previous == current again
    check_motion(s, world_vertices_f32(sd2), cam)
    fresh = Scene(s.desc, device=0, bvh=bvh)
    a, b = s.gbuffer(cam), fresh.gbuffer(cam)
    for k in a:
        assert same_bits(a[k], b[k]), k  # the scene itself still behaves as a fresh build
    s.close(), fresh.close()


def test_motion_guide_flag_refusals_and_device_bytes(rtlib, scene_cache):
    sd = scene_cache("atrium")
    cam = Camera.for_scene(sd, (32, 20))
    plain, upd, keep = Scene(sd, device=0), Scene(sd, device=0, updatable=True), Scene(sd, device=0, updatable=True, keep_previous=True)
    for sc in (plain, upd):
        with pytest.raises(abi.RtError) as e:
            sc.gbuffer_motion(cam)
        assert e.value.status == abi.RT_ERR_INVALID
    assert keep.info().device_bytes - upd.info().device_bytes == 36 * sd.n_triangles
    again = Scene(sd, device=0, updatable=True)
    assert again.info().device_bytes == upd.info().device_bytes
    st_u, st_k = upd.update(instances=spin_about_centre(sd, 2.0)), keep.update(instances=spin_about_centre(sd, 2.0))
    assert st_k.launches == st_u.launches + 1 and st_k.refit_nodes == st_u.refit_nodes  # the test pass before the writing one
    a, b = upd.gbuffer(cam), keep.gbuffer(cam)
    for k in a:
        assert same_bits(a[k], b[k]), k
    bad = Camera.for_scene(sd, (32, 20))
    bad.c.center[0] = 1e12
    with pytest.raises(abi.RtError) as e:
        keep.gbuffer_motion(bad)
    assert e.value.status == abi.RT_ERR_INVALID
    with pytest.raises(abi.RtError) as e:
        keep.gbuffer_motion_device(cam, 1, 1, 1, 0)
    assert e.value.status == abi.RT_ERR_INVALID
    for sc in (plain, upd, keep, again):
        sc.close()


def test_update_waits_for_a_motion_guide_pending_on_another_stream(rtlib, scene_cache):
    """rt_scene_gbuffer_motion_device behind a long kernel on stream A and one on stream B, then rt_scene_update: both launches read the
    scene, and its previous vertices, as they were."""
    import torch
    sd = scene_cache("atrium")
    s = Scene(sd, device=0, updatable=True, keep_previous=True)
    s.update(instances=spin_about_centre(sd, 5.0))
    w, h = 96, 64
    cam = Camera.for_scene(sd, (w, h))
    before = s.gbuffer_motion(cam)
    keys = ("albedo", "normal", "position", "prev_position")
    sa, sb = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    pa = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0") for _ in keys]
    pb = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0") for _ in keys]
    torch.cuda.synchronize()
    with torch.cuda.stream(sa):
        torch.cuda._sleep(200_000_000)  # ~0.1 s of spinning in front of stream A's launch
    s.gbuffer_motion_device(cam, *(p.data_ptr() for p in pa), stream=sa.cuda_stream)
    s.gbuffer_motion_device(cam, *(p.data_ptr() for p in pb), stream=sb.cuda_stream)
    s.update(instances=spin_about_centre(sd, 25.0))
    torch.cuda.synchronize()
    for planes in (pa, pb):
        for k, p in zip(keys, planes):
            assert same_bits(p.cpu().numpy(), before[k]), k
    moved = s.gbuffer_motion(cam)
    assert not same_bits(moved["prev_position"], before["prev_position"]) and not same_bits(moved["position"], before["position"])
    s.close()


# ---- the accumulator ----------------------------------------------------------------------------------------------------------------------
def run_sequence(sd0, w, h, n_frames, params, spin=3.0, spp=2, depth=6, cls=MegakernelRenderer, move_camera=False):
    """Renders n_frames frames (salts 1 .. n), the instances turned by `spin` degrees more per frame (or the camera moved over a scene that is never
    updated), accumulates each on the device and in the model, which carries its own history, and compares the two at every frame. Returns the
    last call's history lengths."""
    s = Scene(sd0, device=0, updatable=True, keep_previous=True)
    r = cls(s, (w, h), depth, spp)
    acc = TemporalAccumulator(0, w, h)
    state, n = None, None
    for f in range(n_frames):
        if f and not move_camera and spin:
            s.update(instances=spin_about_centre(sd0, spin * f))
        if move_camera:
            pos = np.asarray(sd0.camera.position, np.float64) + 0.01 * float(s.scale()) * f * np.array([1.0, 0.3, -0.5])
            cam = Camera((w, h), pos, sd0.camera.direction, sd0.camera.focal_length)
        else:
            cam = Camera.for_scene(sd0, (w, h))
        r.set_frame_seed(f + 1)
        frame = r.render_frame(cam, want_u8=False).rgba_f32
        g = s.gbuffer_motion(cam)
        p = temporal_params(scene_scale=s.scale(), **params)
        kw = dict(max_history=p.max_history, sigma_position=p.sigma_position, cos_normal=p.cos_normal)
        o, b, n = acc.accumulate(frame, g, cam, **kw)
        mo, mb, mn, state = temporal_model(state, frame, g, cam.c, p.max_history, p.sigma_position, p.cos_normal)
        assert same_bits(n, mn), (f, np.argwhere(n != mn)[:4])
        assert same_bits(o, mo), (f, np.argwhere(o.view(np.uint32) != mo.view(np.uint32))[:4])
        assert same_bits(b, mb), f
    acc.close(), r.close(), s.close()
    return n


PARAMS = [dict(), dict(sigma_position=INF), dict(cos_normal=-1.0), dict(max_history=3), dict(max_history=1)]


@pytest.mark.parametrize("params", PARAMS, ids=lambda p: ",".join(f"{k}={v}" for k, v in p.items()) or "defaults")
@pytest.mark.parametrize("name,w,h", [("atrium", 64, 36), ("cornell", 48, 32)])
def test_accumulator_equals_the_model_over_a_sequence(rtlib, scene_cache, name, w, h, params):
    n = run_sequence(scene_cache(name), w, h, 8, params)
    cap = params.get("max_history", TEMPORAL_MAX_HISTORY)
    assert n.max() == min(8, cap)  # (some pixel was followed through all eight frames)
    if cap > 1:
        assert (n >= 2).mean() > 0.5, (n >= 2).mean()  # ... and most of the image found its history


@pytest.mark.parametrize("name,w,h", [("atrium", 64, 36), ("cornell", 48, 32)])
def test_accumulator_follows_a_moving_camera_over_a_static_scene(rtlib, scene_cache, name, w, h):
    n = run_sequence(scene_cache(name), w, h, 8, {}, move_camera=True, cls=WavefrontRenderer)
    assert n.max() == 8 and (n >= 2).mean() > 0.5


@pytest.mark.parametrize("w,h", [(1, 1), (63, 5), (65, 3), (257, 2)])
def test_accumulator_on_partial_tiles(rtlib, scene_cache, w, h):
    run_sequence(scene_cache("cornell"), w, h, 4, {}, spin=2.0)


def test_accumulator_variants_in_place_reset_and_refusals(rtlib, scene_cache):
    import torch
    w, h = 70, 45
    sd = scene_cache("cornell")
    s = Scene(sd, device=0, updatable=True, keep_previous=True)
    r = MegakernelRenderer(s, (w, h), 6, 2)
    acc, dev_acc, inplace_acc = (TemporalAccumulator(0, w, h) for _ in range(3))
    st = torch.cuda.Stream(device=0)
    kw = dict(max_history=TEMPORAL_MAX_HISTORY, sigma_position=float(f32(0.05) * s.scale()), cos_normal=TEMPORAL_COS_NORMAL)
    for f in range(5):
        if f:
            s.update(instances=spin_about_centre(sd, 3.0 * f))
        cam = Camera.for_scene(sd, (w, h))
        r.set_frame_seed(f + 1)
        frame = r.render_frame(cam, want_u8=False).rgba_f32
        g = s.gbuffer_motion(cam)
        o, b, n = acc.accumulate(frame, g, cam, **kw)
        if f:
            assert not same_bits(o, frame)  # history was blended in
        # the _device variant on a non-default stream, in place on the device; the host variant in place: all equal the host call's images
        df = torch.from_numpy(frame).to("cuda:0")
        dg = {k: torch.from_numpy(np.ascontiguousarray(g[k])).to("cuda:0") for k in ("normal", "position", "prev_position")}
        du8 = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
        dn = torch.zeros((h, w), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        dev_acc.accumulate_device(cam, df.data_ptr(), dg["normal"].data_ptr(), dg["position"].data_ptr(), dg["prev_position"].data_ptr(),
                                  df.data_ptr(), du8.data_ptr(), dn.data_ptr(), stream=st.cuda_stream, **kw)
        st.synchronize()
        assert same_bits(df.cpu().numpy(), o) and same_bits(du8.cpu().numpy(), b) and same_bits(dn.cpu().numpy(), n), f
        own = frame.copy()
        fo, fb, fn = inplace_acc.accumulate(own, g, cam, out_f32=own, **kw)
        assert fo is own and same_bits(own, o) and same_bits(fb, b) and same_bits(fn, n), f
        if f == 2:  # single outputs, and the refusals that need an accumulator
            only = TemporalAccumulator(0, w, h)
            f_only, none_b, _ = only.accumulate(frame, g, cam, want_u8=False, **kw)
            none_f, b_only, _ = only.accumulate(frame, g, cam, want_f32=False, **kw)
            assert none_b is None and none_f is None and same_bits(f_only, frame) and b_only.shape == (h, w, 4)
            with pytest.raises(abi.RtError) as e:
                only.accumulate(frame, g, cam, want_f32=False, want_u8=False, **kw)
            assert e.value.status == abi.RT_ERR_INVALID
            wide = Camera.for_scene(sd, (w + 1, h))
            p = temporal_params(**kw)
            ptr = abi.fptr(frame)
            assert only._lib.rt_temporal_accumulate(only.h, C.byref(p), C.byref(wide.c), ptr, ptr, ptr, ptr, ptr, None, None) == abi.RT_ERR_INVALID
            only.close()
        if f == 4:  # (the last frame: the three accumulators' histories part here) after a reset the next output is the input frame
            acc.reset()
            ro, rb, rn = acc.accumulate(frame, g, cam, **kw)
            assert same_bits(ro, frame) and same_bits(rn, np.isfinite(g["position"][..., 3]).astype(f32))
    for a in (acc, dev_acc, inplace_acc):
        a.close()
    r.close(), s.close()


def test_full_hd_sequence_equals_the_model(rtlib, scene_cache):
    n = run_sequence(scene_cache("atrium"), 1920, 1080, 3, {}, spin=1.0, spp=1, depth=4, cls=WavefrontRenderer)
    assert n.max() == 3


# ---- quality -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["atrium", "cornell"])
def test_accumulated_frame_is_closer_to_the_converged_one(rtlib, scene_cache, name):
    """16 frames at 4 spp, salts 1 .. 16, the instances turned by 1 degree per frame: the last accumulated frame against a 1024-spp frame of the
    final scene state, in linear radiance. Asserted on the atrium: RMSE(temporal) < RMSE(raw), an ordering only (a stage that rejected every
    reprojection would return the raw frame and fail the strict test). Reported for both scenes with the same two after 5 a-trous iterations
    at the defaults (§13 explains why the Cornell box resists the spatial filter)."""
    sd0 = scene_cache(name)
    w, h, depth, spp, n_frames = 320, 180, 10, 4, 16
    s = Scene(sd0, device=0, updatable=True, keep_previous=True)
    cam = Camera.for_scene(sd0, (w, h))
    r = MegakernelRenderer(s, (w, h), depth, spp)
    acc = TemporalAccumulator(0, w, h)
    raw = out = g = n = None
    for f in range(n_frames):
        if f:
            s.update(instances=spin_about_centre(sd0, 1.0 * f))
        r.set_frame_seed(f + 1)
        raw = r.render_frame(cam, want_u8=False).rgba_f32
        g = s.gbuffer_motion(cam)
        out, _, n = acc.accumulate(raw, g, cam, want_u8=False, scene_scale=s.scale())
    ref = MegakernelRenderer(s, (w, h), depth, 1024).render_frame(cam, want_u8=False).rgba_f32
    den = Denoiser(0, w, h)
    raw_d, _ = den.denoise(raw, g, want_u8=False, scene_scale=s.scale())
    out_d, _ = den.denoise(out, g, want_u8=False, scene_scale=s.scale())
    e = {k: linear_rmse(v, ref) for k, v in (("raw", raw), ("temporal", out), ("raw+atrous", raw_d), ("temporal+atrous", out_d))}
    print(f"\nquality 320x180 {name}, 16 frames x 4 spp, 1 degree per frame: " + ", ".join(f"{k} {v:.6f}" for k, v in e.items()) +
          f"; mean history {float(n.mean()):.2f}, pixels with history {float((n >= 2).mean()):.3f}")
    if name == "atrium":
        assert e["temporal"] < e["raw"], e
    s.close()


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------------
def cli_spin(ld, centre, deg):
    """host/renderer.h: Scene::spin in its own fp32 operations: every instance of the loaded scene turned by `deg` about the vertical axis
    through `centre`, and the normal matrices from the cofactors."""
    a = deg * 3.14159265358979323846 / 180.0
    c, s = f32(math.cos(a)), f32(math.sin(a))
    z, one = f32(0), f32(1)
    r = np.array([c, z, -s, z, z, one, z, z, s, z, c, z, z, z, z, one], f32)
    cx, cz = f32(centre[0]), f32(centre[2])
    r[12] = cx - (c * cx + s * cz)
    r[14] = cz - ((-s) * cx + c * cz)
    xf0 = np.asarray(ld.transforms, f32).reshape(-1, 16)
    xf = np.zeros_like(xf0)
    for col in range(4):
        for row in range(4):
            v = np.zeros(xf0.shape[0], f32)
            for k in range(4):
                v = v + r[k * 4 + row] * xf0[:, col * 4 + k]
            xf[:, col * 4 + row] = v

    def e(col, row):
        return xf[:, col * 4 + row]
    cof = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            cof[i][j] = e(i1, j1) * e(i2, j2) - e(i1, j2) * e(i2, j1)
    det = (e(0, 0) * cof[0][0] + e(0, 1) * cof[0][1]) + e(0, 2) * cof[0][2]
    nm = np.zeros((xf0.shape[0], 9), f32)
    for i in range(3):
        for j in range(3):
            nm[:, i * 3 + j] = cof[i][j] / det
    return xf, nm


def test_cli_temporal_writes_the_python_path_images(rtlib, tmp_path):
    from PIL import Image
    from rtamd import loader
    glb = REPO / "assets" / "cube.glb"
    w, h, depth, spp, frames, spin, hist = 96, 72, 6, 2, 4, 2.0, 16
    base = [str(EXE), "-w", "-d", str(depth), "-s", str(spp), "--width", str(w), "--height", str(h), "--quiet", "--frames", str(frames),
            "--spin", str(spin)]
    p = subprocess.run([*base, "--temporal", str(hist), "--out", str(tmp_path / "t.png"), str(glb)], capture_output=True, text=True, timeout=300,
                       cwd=tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count(f"Temporal: max history {hist}") == frames and "ms on device 0" in p.stdout, p.stdout
    q = subprocess.run([*base, "--out", str(tmp_path / "p.png"), str(glb)], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert q.returncode == 0 and "Temporal:" not in q.stdout, q.stdout + q.stderr
    ld = loader.load_glb(glb)
    cam = Camera((w, h), ld.camera.position, ld.camera.direction, ld.camera.focal_length)
    for temporal in (True, False):
        s = Scene(ld, device=0, updatable=True, keep_previous=temporal)
        i = s.info()
        centre = [f32(0.5) * (f32(i.bounds_lo[k]) + f32(i.bounds_hi[k])) for k in range(3)]
        r = WavefrontRenderer(s, (w, h), depth, spp)
        acc = TemporalAccumulator(0, w, h)
        for f in range(frames):
            if f:
                s.update(instances=cli_spin(ld, centre, spin * f))
            if temporal:
                r.set_frame_seed(f)
            fr = r.render_frame(cam)
            u8 = fr.rgba_u8
            if temporal:
                _, u8, _ = acc.accumulate(fr.rgba_f32, s.gbuffer_motion(cam), cam, max_history=hist, scene_scale=s.scale())
            cli = np.asarray(Image.open(tmp_path / f"{'t' if temporal else 'p'}_{f:04d}.png"))
            assert same_bits(cli, u8), (temporal, f)  # without --temporal: salt 0, what the CLI always wrote
        acc.close(), r.close(), s.close()
