"""GPU tests of the primary-hit G-buffer (rt_scene_gbuffer[_device]) and the a-trous denoiser (rt_denoise[_device]): both pinned bit for bit to
the numpy float32 models of tests/test_denoise.py, the refusals, the denoiser's quality against a 1024-spp frame and the CLI's --denoise."""
import ctypes as C
import importlib.util
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rtamd import abi
from rtamd.glb_export import export_glb
from rtamd.renderer import Camera, Denoiser, MegakernelRenderer, Scene, WavefrontRenderer, denoise_params

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
EXE = REPO / "sycl-ray-tracer_amd" / "host" / "build" / "raytracer"
f32 = np.float32
INF = float("inf")


def _model_module():
    spec = importlib.util.spec_from_file_location("_denoise_model", Path(__file__).with_name("test_denoise.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_model = _model_module()
gbuffer_model, denoise_model, camera_rays = _model.gbuffer_model, _model.denoise_model, _model.camera_rays


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _status(fn):
    with pytest.raises(abi.RtError) as e:
        fn()
    return e.value.status


SCENES = [("triangle", {}), ("cube", {}), ("cornell", {}), ("atrium", {}), ("voxel", {"detail": 1}), ("atrium_tilted", {}), ("empty", {})]


def _check_gbuffer(scene, sd, cam):
    g = scene.gbuffer(cam)
    org, d = camera_rays(cam.c)
    t, u, v, tri = scene.intersect(org, d)
    m = gbuffer_model(sd, cam.c, t, u, v, tri)
    for k in ("albedo", "normal", "position"):
        assert same_bits(g[k], m[k]), (sd.name, k, np.argwhere(g[k].view(np.uint32) != m[k].view(np.uint32))[:4])
    assert same_bits(g["position"][..., 3].reshape(-1), t)
    return g


@pytest.mark.parametrize("name,kw", SCENES)
def test_gbuffer_equals_the_model(rtlib, scene_cache, name, kw):
    sd = scene_cache(name, **kw)
    s = Scene(sd, device=0)
    sizes = [(1, 1), (7, 5), (65, 3)] + ([(320, 180)] if name in ("atrium", "cornell") else [])
    for w, h in sizes:
        _check_gbuffer(s, sd, Camera.for_scene(sd, (w, h)))
    s.close()


def test_gbuffer_device_variant_and_every_bvh_kind(rtlib, scene_cache):
    import torch
    sd = scene_cache("atrium")
    cam = Camera.for_scene(sd, (160, 90))
    ref = None
    for bvh in (abi.RT_BVH_SAH, abi.RT_BVH_LBVH, abi.RT_BVH_LBVH_GPU):
        s = Scene(sd, device=0, bvh=bvh)
        g = s.gbuffer(cam)
        ref = ref or g
        for k in g:
            assert same_bits(g[k], ref[k]), (bvh, k)
        planes = [torch.full((90, 160, 4), 7.0, dtype=torch.float32, device="cuda:0") for _ in range(3)]
        st = torch.cuda.Stream(device=0)
        s.gbuffer_device(cam, *(p.data_ptr() for p in planes), stream=st.cuda_stream)
        st.synchronize()
        for k, p in zip(("albedo", "normal", "position"), planes):
            assert same_bits(p.cpu().numpy(), g[k]), (bvh, k)
        s.close()
    empty = Scene(scene_cache("empty"), device=0)
    g = empty.gbuffer(Camera.for_scene(scene_cache("empty"), (9, 4)))
    assert np.isinf(g["position"][..., 3]).all() and (g["normal"] == 0).all()


def test_gbuffer_after_an_update_equals_a_fresh_scene(rtlib, scene_cache):
    from test_scene_update import spin_about_centre
    sd = scene_cache("atrium")
    s = Scene(sd, device=0, updatable=True)
    cam = Camera.for_scene(sd, (120, 70))
    s.gbuffer(cam)
    s.update(instances=spin_about_centre(sd, 17.0))
    fresh = Scene(s.desc, device=0)
    a, b = s.gbuffer(cam), fresh.gbuffer(cam)
    for k in a:
        assert same_bits(a[k], b[k]), k
    _check_gbuffer(s, s.desc, cam)
    # an update right behind an enqueued G-buffer: the launch reads the scene as it was
    import torch
    planes = [torch.zeros((70, 120, 4), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    s.gbuffer_device(cam, *(p.data_ptr() for p in planes))
    s.update(instances=spin_about_centre(sd, 40.0))
    torch.cuda.synchronize()
    for k, p in zip(("albedo", "normal", "position"), planes):
        assert same_bits(p.cpu().numpy(), a[k]), k
    s.close(), fresh.close()


def test_update_waits_for_gbuffers_pending_on_several_streams(rtlib, scene_cache):
    """G-buffers enqueued on two streams, the first behind a long kernel, then rt_scene_update: both launches read the scene as it was (the
    update waits for every stream's launch, not only the last one's)."""
    import torch
    from test_scene_update import spin_about_centre
    sd = scene_cache("atrium")
    s = Scene(sd, device=0, updatable=True)
    w, h = 96, 64
    cam = Camera.for_scene(sd, (w, h))
    before = s.gbuffer(cam)
    sa, sb = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    pa = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    pb = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    torch.cuda.synchronize()
    with torch.cuda.stream(sa):
        torch.cuda._sleep(200_000_000)  # ~0.1 s of spinning in front of stream A's G-buffer
    s.gbuffer_device(cam, *(p.data_ptr() for p in pa), stream=sa.cuda_stream)
    s.gbuffer_device(cam, *(p.data_ptr() for p in pb), stream=sb.cuda_stream)
    s.update(instances=spin_about_centre(sd, 25.0))
    torch.cuda.synchronize()
    for planes in (pa, pb):
        for k, p in zip(("albedo", "normal", "position"), planes):
            assert same_bits(p.cpu().numpy(), before[k]), k
    moved = s.gbuffer(cam)
    assert not same_bits(moved["position"], before["position"])  # the update did move the scene
    s.close()


def _synthetic(h, w, seed):
    rng = np.random.default_rng(seed)
    frame = np.ones((h, w, 4), f32)
    frame[..., :3] = rng.random((h, w, 3), dtype=f32) * f32(1.5)
    frame[rng.random((h, w)) < 0.1, :3] = 0
    alb = rng.random((h, w, 4), dtype=f32)
    alb[rng.random((h, w)) < 0.2, :3] = 0
    alb[..., 3] = 0
    nrm = rng.normal(size=(h, w, 4)).astype(f32)
    nrm[..., :3] /= np.linalg.norm(nrm[..., :3], axis=-1, keepdims=True).astype(f32)
    nrm[..., 3] = 0
    pos = (rng.random((h, w, 4), dtype=f32) * f32(4))
    miss = rng.random((h, w)) < 0.25
    pos[miss] = (0, 0, 0, np.inf)
    nrm[miss] = 0
    return frame, {"albedo": alb, "normal": nrm, "position": pos}


SIGMAS = [(0.5, 0.3, 0.4, 0.2), (INF, 0.3, 0.4, 0.2), (0.5, INF, 0.4, 0.2), (0.5, 0.3, INF, 0.2), (0.5, 0.3, 0.4, INF), (1e-3, 1e-6, 1e9, 2.0)]


@pytest.mark.parametrize("h,w", [(1, 1), (1, 257), (17, 9), (64, 64), (197, 333)])
def test_denoise_equals_the_model(rtlib, h, w):
    d = Denoiser(0, w, h)
    for it in (0, 1, 2, 5, 10):
        for si, sig in enumerate(SIGMAS if (h, w) == (17, 9) else SIGMAS[:2]):
            frame, g = _synthetic(h, w, 100 * it + si)
            kw = dict(zip(("sigma_color", "sigma_normal", "sigma_position", "sigma_albedo"), sig))
            f, b = d.denoise(frame, g, iterations=it, **kw)
            mf, mb = denoise_model(frame, g, it, *sig)
            assert same_bits(f, mf), (h, w, it, sig, np.argwhere(f.view(np.uint32) != mf.view(np.uint32))[:4])
            assert same_bits(b, mb), (h, w, it, sig)
    d.close()


def test_infinite_sigma_equals_the_guide_zeroed(rtlib):
    h, w = 33, 70
    frame, g = _synthetic(h, w, 7)
    d = Denoiser(0, w, h)
    base = dict(sigma_color=0.6, sigma_normal=0.4, sigma_position=0.5, sigma_albedo=0.3)
    for k, name in (("albedo", "sigma_albedo"), ("normal", "sigma_normal"), ("position", "sigma_position")):
        a, _ = d.denoise(frame, g, iterations=3, **dict(base, **{name: INF}))
        gz = dict(g)
        gz[k] = g[k].copy()
        gz[k][..., :3] = 0  # position keeps w = t: what tells a hit from a miss
        b, _ = d.denoise(frame, gz, iterations=3, **base)
        assert same_bits(a, b), k
    d.close()


def test_in_place_single_planes_and_device_streams(rtlib):
    import torch
    h, w = 45, 131
    frame, g = _synthetic(h, w, 11)
    d = Denoiser(0, w, h)
    sig = dict(sigma_color=0.7, sigma_normal=0.3, sigma_position=0.6, sigma_albedo=0.4)
    for it in (0, 1, 3):
        ref_f, ref_b = d.denoise(frame, g, iterations=it, **sig)
        f_only, none_b = d.denoise(frame, g, iterations=it, want_u8=False, **sig)
        none_f, b_only = d.denoise(frame, g, iterations=it, want_f32=False, **sig)
        assert none_b is None and none_f is None and same_bits(f_only, ref_f) and same_bits(b_only, ref_b)
        inplace = frame.copy()
        d.denoise(inplace, g, iterations=it, out_f32=inplace, **sig)
        assert same_bits(inplace, ref_f), it
        # device pointers, a non-default stream, in place on the device
        dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in g.items()}
        df = torch.from_numpy(frame).to("cuda:0")
        du8 = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        st = torch.cuda.Stream(device=0)
        d.denoise_device(df.data_ptr(), dev["albedo"].data_ptr(), dev["normal"].data_ptr(), dev["position"].data_ptr(), df.data_ptr(),
                         du8.data_ptr(), stream=st.cuda_stream, iterations=it, **sig)
        st.synchronize()
        assert same_bits(df.cpu().numpy(), ref_f) and same_bits(du8.cpu().numpy(), ref_b), it
    d.close()


def test_refusals(rtlib, scene_cache):
    h, w = 4, 5
    frame, g = _synthetic(h, w, 1)
    d = Denoiser(0, w, h)
    ok = dict(sigma_color=1.0, sigma_normal=1.0, sigma_position=1.0, sigma_albedo=1.0)
    assert _status(lambda: d.denoise(frame, g, iterations=11, **ok)) == abi.RT_ERR_INVALID
    for bad in (0.0, 1e-7, -1.0, float("nan")):
        for name in ok:
            assert _status(lambda: d.denoise(frame, g, iterations=1, **dict(ok, **{name: bad}))) == abi.RT_ERR_INVALID, (name, bad)
    assert _status(lambda: d.denoise(frame, g, iterations=1, want_f32=False, want_u8=False, **ok)) == abi.RT_ERR_INVALID
    p = denoise_params(1, **ok)
    assert d._lib.rt_denoise_device(d.h, C.byref(p), 1, 1, 1, 1, None, None, None) == abi.RT_ERR_INVALID
    d.close()
    sd = scene_cache("cornell")
    s = Scene(sd, device=0)
    cam = Camera.for_scene(sd, (8, 6))
    cam.c.center[0] = 1e9
    assert _status(lambda: s.gbuffer(cam)) == abi.RT_ERR_INVALID
    cam.c.center[0] = float("nan")
    assert _status(lambda: s.gbuffer(cam)) == abi.RT_ERR_INVALID
    cam2 = Camera.for_scene(sd, (8, 6))
    cam2.c.width = 0
    assert _status(lambda: s.gbuffer_device(cam2, 1, 1, 1)) == abi.RT_ERR_INVALID
    assert _status(lambda: s.gbuffer_device(Camera.for_scene(sd, (8, 6)), 0, 1, 1)) == abi.RT_ERR_INVALID
    s.close()


def _linear_rmse(a, ref):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) ** 2 - ref[..., :3].astype(np.float64) ** 2) ** 2)))


@pytest.mark.parametrize("name", ["cornell", "atrium"])
def test_denoised_frame_is_closer_to_the_converged_one(rtlib, scene_cache, name):
    sd = scene_cache(name)
    w, h = 320, 180
    s = Scene(sd, device=0)
    cam = Camera.for_scene(sd, (w, h))
    ref = MegakernelRenderer(s, (w, h), 10, 1024).render_frame(cam, want_u8=False).rgba_f32
    raw = MegakernelRenderer(s, (w, h), 10, 4).render_frame(cam, want_u8=False).rgba_f32
    g = s.gbuffer(cam)
    den, _ = Denoiser(0, w, h).denoise(raw, g, scene_scale=s.scale())
    e_raw, e_den = _linear_rmse(raw, ref), _linear_rmse(den, ref)
    assert e_den < e_raw, (e_den, e_raw)
    s.close()


def test_full_hd_atrium_frame_equals_the_model(rtlib, scene_cache):
    sd = scene_cache("atrium")
    w, h = 1920, 1080
    s = Scene(sd, device=0)
    cam = Camera.for_scene(sd, (w, h))
    raw = WavefrontRenderer(s, (w, h), 10, 2).render_frame(cam, want_u8=False).rgba_f32
    g = s.gbuffer(cam)
    p = denoise_params(3, scene_scale=s.scale())
    kw = dict(sigma_color=p.sigma_color, sigma_normal=p.sigma_normal, sigma_position=p.sigma_position, sigma_albedo=p.sigma_albedo)
    f, b = Denoiser(0, w, h).denoise(raw, g, iterations=3, **kw)
    mf, mb = denoise_model(raw, g, 3, *kw.values())
    assert same_bits(f, mf) and same_bits(b, mb)
    s.close()


def _cli_denoised(glb, tmp_path, name, extra):
    from PIL import Image
    p = subprocess.run([str(EXE), "-w", "-d", "6", "-s", "4", "--width", "96", "--height", "72", "--quiet", "--denoise", "5",
                        "--out", str(tmp_path / name), *extra, str(glb)], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Denoise: 5 iterations" in p.stdout and "ms on device 0" in p.stdout, p.stdout
    return np.asarray(Image.open(tmp_path / name))


def test_cli_denoise_writes_the_python_path_image(rtlib, scene_cache, tmp_path):
    from rtamd import loader
    sd = scene_cache("cornell")
    glb = tmp_path / "cornell.glb"
    export_glb(sd, glb)
    w, h, depth, spp = 96, 72, 6, 4
    cli = _cli_denoised(glb, tmp_path, "d.png", [])
    ld = loader.load_glb(glb)
    s = Scene(ld, device=0)
    cam = Camera((w, h), ld.camera.position, ld.camera.direction, ld.camera.focal_length)
    frame = WavefrontRenderer(s, (w, h), depth, spp).render_frame(cam).rgba_f32
    _, u8 = Denoiser(0, w, h).denoise(frame, s.gbuffer(cam), iterations=5, scene_scale=s.scale())
    assert same_bits(cli, u8)
    # a tiled frame (two tiles, gathered on the root) is denoised there to the same image
    assert same_bits(_cli_denoised(glb, tmp_path, "t.png", ["--devices", "0,0"]), u8)
    s.close()
