"""GPU parity tests (run with -m gpu on an MI355X): the HIP path through the C ABI versus the CPU oracle
on the same seeded inputs and versus the committed golden fixtures.

The bar is BIT-EXACT equality of the fp32 framebuffer, the unorm8 image and the ray count (both sides
execute the same IEEE operations in the same order: DESIGN.md §3), which trivially meets the north-star
tolerance of per-pixel RMSE < 1e-4. Full-size frames, which the oracle cannot finish in seconds, are
covered by size-independent properties plus oracle spot checks of sub-tiles."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest

from rtamd import abi, scenes
from rtamd.renderer import Camera, MegakernelRenderer, Scene, TileComm, WavefrontRenderer, assemble_tiles

REPO = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
NO_TRI = 0xFFFFFFFF
RMSE_TOL = 1e-4  # north-star tolerance; the tests below demand 0 and report the rmse on failure
KINDS = [(MegakernelRenderer, abi.RT_RENDERER_MEGAKERNEL), (WavefrontRenderer, abi.RT_RENDERER_WAVEFRONT)]


def _hw_queues() -> int:
    """GPU_MAX_HW_QUEUES as the library reads it (rt_frame.hip: hw_queues_from_env): a positive number, else HIP's default of 4."""
    try:
        v = int(os.environ.get("GPU_MAX_HW_QUEUES", ""))
    except ValueError:
        v = 0
    return v if v > 0 else 4


HW_QUEUES = _hw_queues()
# the automatic lane count of a launch (pair) per bounce all the way down, or of one fused kernel per bounce: 3, resolved down to
# lanes + 2 <= queues (rt_frame.hip: wf_stream_lanes)
PER_BOUNCE_LANES = 3 if HW_QUEUES >= 5 else 2


@pytest.fixture(scope="module")
def gpu(rtlib):
    n = rtlib.rt_device_count()
    assert n > 0, "GPU tests need a device; the product has no CPU fallback"
    return 0


@pytest.fixture(scope="module")
def gpu_scenes(gpu, scene_cache):
    cache = {}

    def get(name, bvh=abi.RT_BVH_DEFAULT, **kw):
        key = (name, bvh, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = Scene(scene_cache(name, **kw), device=gpu, bvh=bvh)
        return cache[key]

    yield get
    for s in cache.values():
        s.close()


@pytest.fixture(scope="module")
def dev_scenes(gpu, scene_cache, devlib):
    """Scenes in the DEVELOPER build of the library (tests of environment knobs and test hooks; the product build has none)."""
    cache = {}

    def get(name, bvh=abi.RT_BVH_DEFAULT, **kw):
        key = (name, bvh, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = Scene(scene_cache(name, **kw), device=gpu, bvh=bvh, lib=devlib)
        return cache[key]

    yield get
    for s in cache.values():
        s.close()


def _assert_frames_equal(got_f, got_b, got_rays, exp_f, exp_b, exp_rays, what):
    diff = got_f.astype(np.float64) - exp_f.astype(np.float64)
    rmse = float(np.sqrt(np.mean(diff ** 2)))
    nbad = int((got_f != exp_f).any(-1).sum())
    assert got_rays == exp_rays, f"{what}: rays {got_rays} != {exp_rays} (rmse {rmse:.3e}, {nbad} px differ)"
    assert nbad == 0, f"{what}: {nbad} pixels differ, rmse {rmse:.3e} (tolerance {RMSE_TOL})"
    np.testing.assert_array_equal(got_b, exp_b)


# ---- building blocks -----------------------------------------------------------------------------------
def test_device_xorshift(rtlib, gpu, oracle):
    for seed in (1, 0, 2463534242, 0xDEADBEEF):
        out = np.zeros(256, np.float32)
        st = C.c_uint32()
        abi.check(rtlib.rt_probe_xorshift(gpu, seed, 256, abi.fptr(out), C.byref(st)))
        exp, est = oracle.xorshift(seed, 256)
        np.testing.assert_array_equal(out, exp)
        assert st.value == est


def test_short_reciprocal_and_inverse_square_root_are_ieee_on_every_input(rtlib, gpu):
    """rcp_rn / inv_sqrt2 (rt_device.h): v_rcp / v_rsq + a few fma in place of the compiler's IEEE division and square root, inside
    guard ranges found by exhaustive search. The contract (R1) needs RN(1 / x) and RN(1 / RN(sqrt(x))) exactly: compared on the device
    with the IEEE expressions on all 2^32 bit patterns, no input may differ."""
    bad = (C.c_uint64 * 2)()
    abi.check(rtlib.rt_probe_rounding(gpu, bad))
    assert (bad[0], bad[1]) == (0, 0)


def test_device_half_roundtrip(rtlib, gpu, oracle):
    rng = np.random.default_rng(3)
    x = rng.integers(0, 2 ** 32, 300000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    x = x[np.isfinite(x)]
    x = np.concatenate([x, np.array([0.0, -0.0, 65504.0, 65519.99, 65520.0, 1e-8, 2.9802322e-8, 3e-8, 6e-8, 6.1035156e-5,
                                     1.00048828125, np.inf, -np.inf], np.float32),
                        rng.uniform(-2, 2, 200000).astype(np.float32), (rng.uniform(-1, 1, 100000) * 1e-5).astype(np.float32)])
    x = np.ascontiguousarray(x)
    out = np.zeros_like(x)
    bits = np.zeros(x.size, np.uint16)
    abi.check(rtlib.rt_probe_half_roundtrip(gpu, x.size, abi.fptr(x), abi.fptr(out), bits.ctypes.data_as(C.POINTER(C.c_uint16))))
    eo, eb = oracle.half_roundtrip(x)
    np.testing.assert_array_equal(bits, eb)
    np.testing.assert_array_equal(out, eo)


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def test_device_scatter_all_materials(gpu_scenes, oracle, scene_cache):
    """Material::scatter on the device vs the oracle for random inputs, including back-face dielectric
    hits (total internal reflection) and textured albedo lookups with wrapping uv."""
    rng = np.random.default_rng(11)
    for name, kw in (("cornell", {}), ("atrium", {"detail": 1})):
        sd = scene_cache(name, **kw)
        gs, osc = gpu_scenes(name, **kw), oracle.OracleScene(sd)
        n = 20000
        dirs = _unit(rng.normal(size=(n, 3)))
        nrm = _unit(rng.normal(size=(n, 3)))
        uv = rng.uniform(-3, 3, (n, 2)).astype(np.float32)
        uv[:50] = np.array([[0.0, 0.0], [1.0, 1.0], [-1.0, 2.0], [0.999999, 0.5], [1e-9, -1e-9]] * 10, np.float32)
        seeds = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        seeds[:3] = (0, 1, 0xFFFFFFFF)
        for m in range(len(sd.materials)):
            g = gs.scatter(m, dirs, nrm, uv, seeds)
            e = osc.scatter(m, dirs, nrm, uv, seeds)
            np.testing.assert_array_equal(g[0], e[0], err_msg=f"{name} material {m}: ok flag")
            np.testing.assert_array_equal(g[3], e[3], err_msg=f"{name} material {m}: rng state")
            if sd.materials[m].type != abi.RT_MAT_NONE:
                np.testing.assert_array_equal(g[1], e[1], err_msg=f"{name} material {m}: direction")
                np.testing.assert_array_equal(g[2], e[2], err_msg=f"{name} material {m}: attenuation")


@pytest.mark.parametrize("name,kw,brute", [("triangle", {}, True), ("cube", {}, True), ("cornell", {}, True),
                                            ("atrium", {"detail": 1}, True), ("atrium", {"detail": 2}, False), ("voxel", {"detail": 1}, True),
                                            ("atrium_tilted", {"detail": 1}, True)])  # the last one: pre-split triangles sit in several leaves
@pytest.mark.parametrize("bvh", [abi.RT_BVH_LBVH, abi.RT_BVH_SAH, abi.RT_BVH_LBVH_GPU])
def test_intersect_batch_equals_oracle(gpu_scenes, oracle, scene_cache, name, kw, brute, bvh):
    """rtcIntersect1 replacement: BVH traversal on the GPU == brute force over all triangles on the CPU,
    for camera rays, random interior rays and rays that start ON surfaces (the self-hit / tnear case)."""
    sd = scene_cache(name, **kw)
    gs, osc = gpu_scenes(name, bvh=bvh, **kw), oracle.OracleScene(sd)
    rng = np.random.default_rng(5)
    n = 6000 if brute and sd.n_triangles > 5000 else 20000
    tw = sd.world_triangles()
    lo, hi = tw.reshape(-1, 3).min(0), tw.reshape(-1, 3).max(0)
    org = rng.uniform(lo - 0.1 * (hi - lo) - 0.5, hi + 0.1 * (hi - lo) + 0.5, (n, 3)).astype(np.float32)
    dirs = rng.normal(size=(n, 3)).astype(np.float32)
    dirs[: n // 4] *= 1e-2   # short unnormalised directions (scattered rays are unnormalised)
    dirs = dirs.astype(np.float16).astype(np.float32)  # directions always pass through half storage
    # rays that start on triangle surfaces
    k = n // 3
    ti = rng.integers(0, sd.n_triangles, k)
    b = rng.dirichlet((1, 1, 1), k)
    org[:k] = np.einsum("ij,ijk->ik", b, tw[ti]).astype(np.float32)
    # axis-aligned directions with exact zeros (0 * inf in the slab test)
    dirs[k: k + 60] = np.tile(np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [0, 1, 1], [-1, 0, 1], [1, 1, 0]], np.float32), (10, 1))
    gt, gu, gv, gtri = gs.intersect(org, dirs)
    et, eu, ev, etri = osc.intersect(org, dirs, use_bvh=not brute)
    assert (etri != NO_TRI).sum() > n // 50
    np.testing.assert_array_equal(gtri, etri)
    np.testing.assert_array_equal(gt, et)
    np.testing.assert_array_equal(gu, eu)
    np.testing.assert_array_equal(gv, ev)


# ---- whole renders -------------------------------------------------------------------------------------
# (every fixture of make_golden.py; host_walks.npz is make_host_walks.py's, held by tests/test_host_walks.py)
@pytest.mark.parametrize("case", sorted(p.stem for p in GOLDEN.glob("*.npz") if p.stem != "host_walks"))
def test_render_equals_golden_fixtures(gpu_scenes, case):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", GOLDEN / "make_golden.py")
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    scene, kw, w, h, spp, depth = mg.CASES[case]
    g = np.load(GOLDEN / f"{case}.npz")
    gs = gpu_scenes(scene, **kw)
    cam = Camera.for_scene(gs.desc, (w, h))
    for cls, tag in ((MegakernelRenderer, "mega"), (WavefrontRenderer, "wave")):
        r = cls(gs, (w, h), depth, spp)
        fr = r.render_frame(cam)
        _assert_frames_equal(fr.rgba_f32, fr.rgba_u8, fr.rays, g[f"{tag}_f32"], g[f"{tag}_u8"], int(g[f"{tag}_rays"]), f"{case}/{tag}")
        r.close()
    # primary-hit table through the intersect entry point
    X, Y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32), indexing="xy")
    c = cam.c
    p00, du, dv, ce = (np.array(list(v), np.float32) for v in (c.pixel00, c.delta_u, c.delta_v, c.center))
    dirs = (((p00 + X[..., None] * du) + Y[..., None] * dv) - ce).astype(np.float32).reshape(-1, 3)
    t, u, v, tri = gs.intersect(np.broadcast_to(ce, dirs.shape).copy(), dirs)
    np.testing.assert_array_equal(tri, g["hit_tri"])
    np.testing.assert_array_equal(t, g["hit_t"])
    np.testing.assert_array_equal(u, g["hit_u"])
    np.testing.assert_array_equal(v, g["hit_v"])


# BASELINE.json configs, at sizes the oracle finishes in seconds (full sizes: properties test below)
CONFIGS = [
    ("triangle", {}, 256, 256, 1, 10, False),     # config 1 at full size
    ("cube", {}, 256, 256, 4, 10, False),         # config 2 (512x512x16 at reduced size)
    ("cornell", {}, 160, 160, 8, 10, False),      # config 3 (emissive -> wavefront clamp differs)
    ("atrium", {"detail": 2}, 240, 136, 2, 10, True),  # configs 4/5 geometry class, oracle BVH
    ("atrium_tilted", {"detail": 1}, 200, 112, 3, 10, True),  # large diagonal triangles: the SAH builder pre-splits them (one triangle, several leaves)
    ("voxel", {"detail": 1}, 200, 112, 3, 10, True),  # the second workload class (the reference's minecraft.glb): axis-aligned unit faces, open sky
    ("cornell", {}, 97, 61, 3, 1, False),         # odd size (partial 8x8 tiles), depth 1
    ("cube", {}, 64, 40, 2, 16, False),           # depth 16 as in config 5
]


@pytest.mark.parametrize("name,kw,w,h,spp,depth,use_bvh", CONFIGS)
@pytest.mark.parametrize("cls,kind", KINDS)
def test_render_equals_oracle(gpu_scenes, oracle, scene_cache, cls, kind, name, kw, w, h, spp, depth, use_bvh):
    sd = scene_cache(name, **kw)
    gs = gpu_scenes(name, **kw)
    r = cls(gs, (w, h), depth, spp)
    fr = r.render_frame(Camera.for_scene(sd, (w, h)))
    r.close()
    osc = oracle.OracleScene(sd)
    ocam = oracle.camera(w, h, sd.camera.position, sd.camera.direction, sd.camera.focal_length)
    f, b, rays = osc.render(ocam, kind, depth, spp, use_bvh=use_bvh)
    _assert_frames_equal(fr.rgba_f32, fr.rgba_u8, fr.rays, f, b, rays, f"{name} {w}x{h} {spp}spp d{depth} {cls.__name__}")


@pytest.mark.parametrize("seed_mode", [abi.RT_SEED_WAVEFRONT, abi.RT_SEED_MEGAKERNEL])
def test_megakernel_equals_wavefront_with_equal_seeds(gpu_scenes, seed_mode):
    """Appendix A-E3 on the device: equal seeds, no sample above 1 -> identical frames and ray counts."""
    for name in ("triangle", "cube"):
        gs = gpu_scenes(name)
        w, h = 200, 120
        cam = Camera.for_scene(gs.desc, (w, h))
        a = MegakernelRenderer(gs, (w, h), 10, 6, seed_mode)
        b = WavefrontRenderer(gs, (w, h), 10, 6, seed_mode)
        fa, fb = a.render_frame(cam), b.render_frame(cam)
        assert fa.rays == fb.rays
        np.testing.assert_array_equal(fa.rgba_f32, fb.rgba_f32)
        np.testing.assert_array_equal(fa.rgba_u8, fb.rgba_u8)
        a.close(), b.close()


def test_gpu_built_lbvh_is_valid_and_fast(gpu_scenes, scene_cache):
    """RT_BVH_LBVH_GPU: Morton + radix sort + Karras + refit + BVH4 collapse on the device. The downloaded tree
    passes the host's structural check; the build beats the host SAH build."""
    import time
    sd = scene_cache("atrium", detail=4)
    Scene(sd, 0, abi.RT_BVH_LBVH_GPU).close()  # (first use: rocPRIM's kernels are loaded, the device allocator warms up)

    def best_of_three(bvh):
        best, sc = None, None
        for _ in range(3):
            if sc is not None:
                sc.close()
            t0 = time.perf_counter()
            sc = Scene(sd, 0, bvh)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best, sc

    t_gpu, g = best_of_three(abi.RT_BVH_LBVH_GPU)
    g.check_bvh()
    info = g.info()
    assert info.n_triangles == sd.n_triangles and info.max_leaf_tris == 1 and info.n_nodes > sd.n_triangles // 8
    t_host, h = best_of_three(abi.RT_BVH_SAH)
    print(f"scene create: GPU LBVH {t_gpu*1e3:.1f} ms, host SAH {t_host*1e3:.1f} ms")
    # (wall-clock best-of-three on a box that may be shared: a wide margin; measured 60 vs 152 ms)
    assert t_gpu < 2.0 * t_host, f"the device build ({t_gpu*1e3:.1f} ms) should not lose to the host SAH build ({t_host*1e3:.1f} ms) by 2x"
    g.close(), h.close()
    for small in ("triangle", "cube", "empty"):  # fewer than 8 triangles: served by the host builder
        s2 = Scene(scene_cache(small), 0, abi.RT_BVH_LBVH_GPU)
        s2.check_bvh()
        s2.close()


@pytest.mark.parametrize("cls,kind", KINDS)
def test_bvh_builder_does_not_change_the_image(gpu_scenes, cls, kind):
    frames = []
    for bvh in (abi.RT_BVH_LBVH, abi.RT_BVH_SAH, abi.RT_BVH_LBVH_GPU):
        gs = gpu_scenes("atrium", bvh=bvh, detail=2)
        r = cls(gs, (320, 180), 10, 3)
        frames.append(r.render_frame(Camera.for_scene(gs.desc, (320, 180))))
        r.close()
    for f in frames[1:]:
        assert frames[0].rays == f.rays
        np.testing.assert_array_equal(frames[0].rgba_f32, f.rgba_f32)


@pytest.mark.parametrize("cls,kind", KINDS)
def test_presplit_triangles_do_not_change_the_image(oracle, scene_cache, monkeypatch, devlib, cls, kind):
    """The SAH builder's pre-splitting of large diagonal triangles puts one triangle into several leaves. The closest hit is min t with ties
    to the lowest triangle index, and the same triangle tested twice gives the same t: frame, unorm8 image and ray count must be those of
    the tree without splits — and the oracle's."""
    sd = scene_cache("atrium_tilted", detail=1)
    w, h, depth, spp = 224, 126, 10, 3
    cam = Camera.for_scene(sd, (w, h))
    frames = []
    for budget in ("0", "0.3", "1.5"):
        monkeypatch.setenv("RT_BVH_SPLIT_BUDGET", budget)  # read by rt_scene_create of the developer build
        gs = Scene(sd, 0, abi.RT_BVH_SAH, lib=devlib)
        info = gs.info()
        assert (info.n_split_triangles > 0) == (budget != "0") and info.n_leaf_records >= sd.n_triangles
        r = cls(gs, (w, h), depth, spp)
        frames.append(r.render_frame(cam))
        r.close()
        gs.close()
    f, b, rays = _oracle_frame(oracle, sd, w, h, kind, depth, spp, use_bvh=True)
    for fr in frames:
        _assert_frames_equal(fr.rgba_f32, fr.rgba_u8, fr.rays, f, b, rays, "pre-split tree")


@pytest.mark.parametrize("cls,kind", KINDS)
@pytest.mark.parametrize("world,strip", [(2, 8), (3, 8), (8, 8), (4, 16)])
def test_tile_split_union_equals_full_frame(gpu_scenes, cls, kind, world, strip):
    """Multi-GPU tile split, all ranks rendered on this one GPU: the de-interleaved union of the tiles is
    bit-identical to the single-GPU frame and the ray counts add up (seeds use global pixel coordinates)."""
    gs = gpu_scenes("cornell")
    w, h = 120, 93  # not a multiple of the strip height
    cam = Camera.for_scene(gs.desc, (w, h))
    r = cls(gs, (w, h), 10, 3)
    full = r.render_frame(cam)
    parts, rays = [], 0
    for rank in range(world):
        r.set_tile(rank, world, strip)
        rows = r.global_rows()
        assert all((y // strip) % world == rank for y in rows) and len(rows) == r.local_rows
        fr = r.render_frame(cam)
        parts.append(fr.rgba_f32)
        rays += fr.rays
    r.close()
    assert rays == full.rays
    np.testing.assert_array_equal(assemble_tiles(parts, h, world, strip), full.rgba_f32)


@pytest.mark.parametrize("cls,kind", KINDS)
@pytest.mark.parametrize("devices", [(0, 0, 0), (0,), (0, 0, 0, 0, 0, 0, 0, 0)])
def test_native_frame_gather_equals_the_single_device_frame(gpu_scenes, oracle, cls, kind, devices):
    """rt_comm_create / rt_frame_gather (the library's own multi-GPU gather): every tile is rendered into its
    renderer's device buffer, the strips are brought to the root device and de-interleaved there; the frame that comes back is
    bit-identical to the single-device frame AND to the oracle, and the ray counts add up. On this one-GPU box a list that names
    device 0 several times takes the device-copy path (RCCL allows one rank per device); the one-rank list (0,) takes the RCCL
    path itself: ncclCommInitAll + grouped ncclGather on a communicator of size 1. Image height 93 is not a multiple of the
    strip height, so the last strip is short and the ranks own different numbers of rows (ncclGather sends padded tiles)."""
    gs = gpu_scenes("cornell")
    w, h, depth, spp = 120, 93, 6, 3
    cam = Camera.for_scene(gs.desc, (w, h))
    ref = cls(gs, (w, h), depth, spp)
    full = ref.render_frame(cam)
    ref.close()
    n = len(devices)
    comm = TileComm(devices)
    assert comm.uses_rccl == (n == 1)
    rs = []
    for k in range(n):
        r = cls(gs, (w, h), depth, spp)
        r.set_tile(k, n, 8)
        rs.append(r)
    for _ in range(2):  # the communicator and its root buffers are reusable
        f, b, rays = comm.render_and_gather(rs, cam)
        assert rays == full.rays
        np.testing.assert_array_equal(f, full.rgba_f32)
        np.testing.assert_array_equal(b, full.rgba_u8)
    sd = gs.desc
    of, ob, orays = oracle.OracleScene(sd).render(oracle.camera(w, h, sd.camera.position, sd.camera.direction, sd.camera.focal_length), kind, depth, spp)
    _assert_frames_equal(f, b, rays, of, ob, orays, f"gathered frame, {n} tiles")
    # only the u8 plane (what the CLI asks for)
    f2, b2, _ = comm.render_and_gather(rs, cam, want_f32=False)
    assert f2 is None
    np.testing.assert_array_equal(b2, full.rgba_u8)
    # a renderer that is not tile (i, n) of the frame is refused, not gathered
    if n > 1:
        rs[1].set_tile(0, n, 8)
        with pytest.raises(abi.RtError):
            comm.render_and_gather(rs, cam)
    for r in rs:
        r.close()
    comm.close()


ALL_BOUNCES = abi.RT_SCHED_ALL_BOUNCES


def _oracle_frame(oracle, sd, w, h, kind, depth, spp, **kw):
    ocam = oracle.camera(w, h, sd.camera.position, sd.camera.direction, sd.camera.focal_length)
    return oracle.OracleScene(sd).render(ocam, kind, depth, spp, **kw)


@pytest.mark.parametrize("requeue", [1, 0])
@pytest.mark.parametrize("samples_per_launch", [1, 2, 3, 5, 64])
def test_wavefront_streaming_samples_keep_the_frame(gpu_scenes, oracle, samples_per_launch, requeue):
    """rt_schedule.samples_per_launch (finish_depth 0): k_wf_finish renders that many samples of every pixel per launch instead of all
    of them. requeue = 1: the lane whose path has ended hands the pixel, with its RNG word, to a device-wide dynamic queue and
    any idle lane generates its next camera ray (breadth first); requeue = 0: the lane keeps the pixel and generates the next camera
    ray itself (depth first). 5 samples in chunks of 1, 2, 3, 5 and 64 (= all in one launch; 2 and 3 leave a shorter last chunk):
    frame, unorm8 image and ray count equal the oracle's WavefrontRenderer, with Russian roulette and on an odd tile too — and the
    launch counts the library reports are those of the schedule asked for."""
    for name, kw, (w, h), depth, spp in (("cornell", {}, (96, 64), 8, 5), ("atrium", {"detail": 1}, (192, 108), 10, 5), ("cube", {}, (64, 40), 1, 5)):
        gs = gpu_scenes(name, **kw)
        sd = gs.desc
        cam = Camera.for_scene(sd, (w, h))
        use_bvh = name == "atrium"
        r = WavefrontRenderer(gs, (w, h), depth, spp)
        r.set_schedule(finish_depth=0, samples_per_launch=samples_per_launch, requeue=requeue)
        got = r.render_frame(cam)
        c = min(samples_per_launch, spp)
        n_launches = -(-spp // c)
        assert got.stream_lanes == 2 and got.samples_per_launch == c and got.finish_depth == 0
        assert got.kernels["wf_finish"] == 2 * n_launches and got.kernels["wf_generate"] == 2 * n_launches
        with_queue = sum(1 for s0 in range(0, spp, c) if min(c, spp - s0) > 1)  # launches that render more than one sample use the dynamic queue
        assert got.kernels["wf_finish_requeue"] == (2 * with_queue if requeue else 0)
        assert got.kernels["wf_extend"] == got.kernels["wf_shade"] == 0
        f, b, rays = _oracle_frame(oracle, sd, w, h, abi.RT_RENDERER_WAVEFRONT, depth, spp, use_bvh=use_bvh)
        _assert_frames_equal(got.rgba_f32, got.rgba_u8, got.rays, f, b, rays, f"{name} samples_per_launch={samples_per_launch}")
        again = r.render_frame(cam)
        _assert_frames_equal(again.rgba_f32, again.rgba_u8, again.rays, f, b, rays, f"{name} second frame")
        r.set_russian_roulette(2)
        got_rr = r.render_frame(cam)
        f, b, rays = _oracle_frame(oracle, sd, w, h, abi.RT_RENDERER_WAVEFRONT, depth, spp, use_bvh=use_bvh, rr_start=2)
        _assert_frames_equal(got_rr.rgba_f32, got_rr.rgba_u8, got_rr.rays, f, b, rays, f"{name} samples_per_launch={samples_per_launch} rr")
        r.set_russian_roulette(0)
        r.set_tile(1, 3, 8)
        tile = r.render_frame(cam)
        f, b, rays = _oracle_frame(oracle, sd, w, h, abi.RT_RENDERER_WAVEFRONT, depth, spp, use_bvh=use_bvh, rank=1, world=3, strip_rows=8)
        _assert_frames_equal(tile.rgba_f32, tile.rgba_u8, tile.rays, f, b, rays, f"{name} samples_per_launch={samples_per_launch} tile 1/3")
        r.close()


SCHEDULES = [dict(samples_per_launch=1, stream_lanes=2), dict(samples_per_launch=1, stream_lanes=3), dict(samples_per_launch=1, requeue=0),
             dict(stream_lanes=1, samples_per_launch=2), dict(stream_lanes=4, samples_per_launch=3, requeue=1), dict(finish_depth=2, stream_lanes=1),
             dict(stream_lanes=2), dict(stream_lanes=3, cost_order=1), dict(finish_depth=ALL_BOUNCES, stream_lanes=1), dict(finish_depth=ALL_BOUNCES, hip_graph=True),
             dict(finish_depth=ALL_BOUNCES, fused_bounce=True), dict(finish_depth=ALL_BOUNCES, fused_bounce=True, stream_lanes=1), dict(finish_depth=3, fused_bounce=True, stream_lanes=3)]


@pytest.mark.parametrize("sched", SCHEDULES, ids=lambda e: ",".join(f"{k}={v if v != ALL_BOUNCES else 'all'}" for k, v in e.items()))
def test_wavefront_schedule_knobs_keep_the_frame(gpu_scenes, oracle, sched):
    """rt_renderer_set_schedule: stream lanes x samples per launch x hand-over form x per-bounce depth, in combination (one launch per
    frame on several stream lanes included). Whatever the combination, frame, unorm8 image and ray count are the oracle's, and the
    stats name the kernels that ran."""
    for name, kw, (w, h), depth, spp in (("cornell", {}, (96, 64), 8, 5), ("atrium", {"detail": 1}, (200, 120), 10, 4)):
        gs = gpu_scenes(name, **kw)
        sd = gs.desc
        cam = Camera.for_scene(sd, (w, h))
        r = WavefrontRenderer(gs, (w, h), depth, spp)
        r.set_schedule(**sched)
        back = r.get_schedule()
        assert all(getattr(back, k) == int(v) for k, v in sched.items())
        got = r.render_frame(cam)
        # automatic: 1 for the one-launch schedule, PER_BOUNCE_LANES for a launch (pair) per bounce all the way down or one fused kernel per
        # bounce, else 2
        lanes = sched.get("stream_lanes", 0) or (1 if sched.get("samples_per_launch", 0) == 0 and sched.get("finish_depth", 0) == 0
                                                else PER_BOUNCE_LANES if sched.get("fused_bounce") or sched.get("finish_depth", 0) >= depth else 2)
        assert got.hw_queues == HW_QUEUES
        assert got.stream_lanes == lanes and got.finish_depth == min(sched.get("finish_depth", 0), depth)
        assert got.kernels["wf_init"] == got.kernels["wf_resolve"] == lanes
        fused = bool(sched.get("fused_bounce"))  # one SHOOT launch per bounce instead of the EXTEND + SHADE pair
        assert got.kernels["wf_extend"] == got.kernels["wf_shade"] == (0 if fused else lanes * spp * got.finish_depth)
        assert got.kernels["wf_shoot"] == (lanes * spp * got.finish_depth if fused else 0)
        assert (got.kernels["wf_finish"] > 0) == (got.finish_depth < depth)
        assert sum(got.kernels.values()) - got.kernels["wf_shade_reorder"] - got.kernels["wf_shade_matsort"] - got.kernels["wf_finish_requeue"] == got.launches
        f, b, rays = _oracle_frame(oracle, sd, w, h, abi.RT_RENDERER_WAVEFRONT, depth, spp, use_bvh=(name == "atrium"))
        _assert_frames_equal(got.rgba_f32, got.rgba_u8, got.rays, f, b, rays, f"{name} {sched}")
        r.set_tile(2, 3, 8)
        tile = r.render_frame(cam)
        f, b, rays = _oracle_frame(oracle, sd, w, h, abi.RT_RENDERER_WAVEFRONT, depth, spp, use_bvh=(name == "atrium"), rank=2, world=3, strip_rows=8)
        _assert_frames_equal(tile.rgba_f32, tile.rgba_u8, tile.rays, f, b, rays, f"{name} {sched} tile 2/3")
        r.set_russian_roulette(2)  # the roulette's extra draw sits between shading and the hand-over to the next queue, in every schedule
        rr = r.render_frame(cam)
        f, b, rays = _oracle_frame(oracle, sd, w, h, abi.RT_RENDERER_WAVEFRONT, depth, spp, use_bvh=(name == "atrium"), rank=2, world=3, strip_rows=8, rr_start=2)
        _assert_frames_equal(rr.rgba_f32, rr.rgba_u8, rr.rays, f, b, rays, f"{name} {sched} tile 2/3, roulette")
        r.close()


def test_schedule_environment_shim_maps_onto_the_api(dev_scenes, gpu_scenes, oracle, monkeypatch):
    """The RT_WF_* environment variables (the DEVELOPER build's, for sweep scripts) only fill the initial rt_schedule at rt_renderer_create:
    the same schedules run as through the API, and the stats say so. The PRODUCT build does not read them."""
    gs = dev_scenes("cornell")
    sd = gs.desc
    w, h, depth, spp = 96, 64, 6, 4
    cam = Camera.for_scene(sd, (w, h))
    f, b, rays = _oracle_frame(oracle, sd, w, h, abi.RT_RENDERER_WAVEFRONT, depth, spp)
    cases = [({"RT_WF_FINISH_DEPTH": "99", "RT_WF_REORDER": "1"}, dict(finish_depth=99, reorder=1), ("wf_shade_reorder", PER_BOUNCE_LANES * spp * depth)),
             ({"RT_WF_STREAMS": "3"}, dict(stream_lanes=3, samples_per_launch=1), ("wf_finish", 3 * spp)),
             ({"RT_WF_REQUEUE": "0"}, dict(requeue=0, samples_per_launch=1), ("wf_finish", 2 * spp)),
             ({"RT_WF_SAMPLES_PER_LAUNCH": "2"}, dict(samples_per_launch=2), ("wf_finish_requeue", 2 * 2)),
             ({"RT_WF_LPT": "0"}, dict(cost_order=0), ("wf_finish", 1)), ({}, dict(finish_depth=0, samples_per_launch=0, stream_lanes=0), ("wf_finish", 1))]
    for env, want, (kernel, count) in cases:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        r = WavefrontRenderer(gs, (w, h), depth, spp)
        for k in env:
            monkeypatch.delenv(k)
        sc = r.get_schedule()
        assert all(getattr(sc, k) == v for k, v in want.items()), (env, {k: getattr(sc, k) for k in want})
        got = r.render_frame(cam)
        assert got.kernels[kernel] == count, (env, got.kernels)
        _assert_frames_equal(got.rgba_f32, got.rgba_u8, got.rays, f, b, rays, f"env {env}")
        r.close()
    monkeypatch.setenv("RT_WF_FINISH_DEPTH", "99")
    monkeypatch.setenv("RT_WF_STREAMS", "3")
    r = WavefrontRenderer(gpu_scenes("cornell"), (w, h), depth, spp)  # the product build: deaf to them
    sc = r.get_schedule()
    assert sc.finish_depth == 0 and sc.stream_lanes == 0
    r.close()


def test_failed_reallocation_leaves_a_renderer_that_says_so(dev_scenes, oracle, monkeypatch, devlib):
    """rt_renderer_set_schedule / rt_renderer_set_tile free and re-allocate the tile's queues. If an allocation fails part-way (injected:
    RT_INJECT_ALLOC_FAILURE=k fails the k-th one as out of memory) the renderer must not keep half-built lanes that the next frame would
    launch on: the call reports RT_ERR_OOM, the schedule / tile on record stay the last ones that worked, every frame entry point
    refuses the renderer with an error code — the frame gather too — and a later successful call makes it whole again: same frame as before.
    (The hook exists in the developer build only.)"""
    gs = dev_scenes("cornell")
    sd = gs.desc
    w, h, depth, spp = 64, 48, 5, 2
    cam = Camera.for_scene(sd, (w, h))
    for cls, kind in ((WavefrontRenderer, abi.RT_RENDERER_WAVEFRONT), (MegakernelRenderer, abi.RT_RENDERER_MEGAKERNEL)):
        f, b, rays = _oracle_frame(oracle, sd, w, h, kind, depth, spp)
        r = cls(gs, (w, h), depth, spp)
        for k in ((1, 2, 3) if cls is MegakernelRenderer else (1, 2, 3, 6, 9, 15, 27)):  # (odd: the 3-lane schedule's ~40 allocations; even: the default's ~10)
            monkeypatch.setenv("RT_INJECT_ALLOC_FAILURE", str(k))
            with pytest.raises(abi.RtError) as e:
                if cls is WavefrontRenderer and k % 2:
                    r.set_schedule(finish_depth=ALL_BOUNCES, stream_lanes=3)
                else:
                    r.set_tile(0, 2, 8)
            assert e.value.status == abi.RT_ERR_OOM, e.value
            monkeypatch.delenv("RT_INJECT_ALLOC_FAILURE")
            sc = r.get_schedule()
            assert sc.finish_depth == 0 and sc.stream_lanes == 0  # the schedule on record: the last one that worked
            comm = TileComm([0], lib=devlib)
            for call in (lambda: r.render_frame(cam), lambda: r.begin_frame(cam), lambda: comm.gather_begin([r])):
                with pytest.raises(abi.RtError) as e:
                    call()
                assert e.value.status == abi.RT_ERR_INVALID and "no buffers" in str(e.value)
            comm.close()
            r.set_tile(0, 1, 8)  # whole again
            got = r.render_frame(cam)
            _assert_frames_equal(got.rgba_f32, got.rgba_u8, got.rays, f, b, rays, f"{cls.__name__} after failure {k}")
        r.close()


def test_library_loaded_after_hip_is_up_resolves_its_stream_lanes(gpu_scenes, oracle):
    """A host that initialised HIP before it loaded the library, with the hardware queues its environment gives it (HIP's four when
    GPU_MAX_HW_QUEUES is not set). The library does not touch the environment (round 3 did, from a constructor): it reads the host's
    setting, resolves the per-bounce schedules' automatic three stream lanes down to what the queues serve (lanes + 2 <= queues), says so in
    rt_stats, and renders the same frame. Run in a child process (this one has loaded the library already): torch brings HIP up first,
    THEN the library is loaded."""
    gs = gpu_scenes("cornell")
    sd = gs.desc
    w, h, depth, spp = 96, 64, 6, 4
    f, b, rays = _oracle_frame(oracle, sd, w, h, abi.RT_RENDERER_WAVEFRONT, depth, spp)
    code = f"""
import hashlib, json, sys
sys.path.insert(0, {str(REPO)!r}); sys.path.insert(0, {str(REPO / 'sycl-ray-tracer_amd')!r})
import torch
torch.cuda.init(); x = torch.zeros(4, device='cuda'); torch.cuda.synchronize()   # HIP is up, with its default queues
from rtamd import abi, scenes
from rtamd.renderer import Camera, Scene, WavefrontRenderer
sd = scenes.get_scene('cornell'); sc = Scene(sd, 0); cam = Camera.for_scene(sd, ({w}, {h}))
out = {{}}
for name, kw in (('split', dict(finish_depth=abi.RT_SCHED_ALL_BOUNCES)), ('fused', dict(finish_depth=abi.RT_SCHED_ALL_BOUNCES, fused_bounce=True)),
                 ('asked3', dict(finish_depth=abi.RT_SCHED_ALL_BOUNCES, stream_lanes=3))):
    r = WavefrontRenderer(sc, ({w}, {h}), {depth}, {spp}); r.set_schedule(**kw)
    fr = r.render_frame(cam)
    out[name] = dict(lanes=fr.stream_lanes, queues=fr.hw_queues, rays=fr.rays, f32=hashlib.sha1(fr.rgba_f32.tobytes()).hexdigest(),
                     u8=hashlib.sha1(fr.rgba_u8.tobytes()).hexdigest(), extend=fr.kernels['wf_extend'], shoot=fr.kernels['wf_shoot'])
    r.close()
print('RESULT ' + json.dumps(out))
"""
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    want_f32, want_u8 = hashlib.sha1(f.tobytes()).hexdigest(), hashlib.sha1(b.tobytes()).hexdigest()
    for name, o in out.items():
        assert o["queues"] == HW_QUEUES, (name, o)               # what the library saw: the host's setting, or HIP's default
        assert o["lanes"] == (3 if name == "asked3" else PER_BOUNCE_LANES), (name, o)  # automatic: resolved down; explicit: the caller's business
        assert (o["rays"], o["f32"], o["u8"]) == (rays, want_f32, want_u8), (name, o)
    assert out["split"]["extend"] == PER_BOUNCE_LANES * spp * depth and out["fused"]["shoot"] == PER_BOUNCE_LANES * spp * depth


@pytest.mark.parametrize("env", [{"RT_WF_SHOOT_TAIL": "0"}, {"RT_WF_SHOOT_TAIL": "0", "RT_WF_SHOOT_CHUNK": "32"}, {"RT_WF_SHOOT_STATIC_PCT": "0", "RT_WF_SHOOT_CHUNK": "16"},
                                 {"RT_WF_SHOOT_STATIC_PCT": "100"}, {"RT_WF_SHOOT_STATIC_PCT": "40", "RT_WF_SHOOT_CHUNK": "1024"}, {}])
def test_shoot_queue_claims_keep_the_frame(dev_scenes, oracle, monkeypatch, env):
    """SHOOT's input claims (rt_frame.hip: wf_shoot_tail): a static share of the queue in equal parts plus guided claims of what is left
    (the default), fixed chunks (RT_WF_SHOOT_TAIL=0; developer build), the extremes of the static share and of the claim size — which ray a wave traces
    never changes a pixel: frame, unorm8 image and ray count are the oracle's on a frame whose queues are longer than one claim per wave
    and on one that fits a single wave's static part, on one stream lane and on three."""
    for name, kw, (w, h), depth, spp in (("atrium", {"detail": 1}, (512, 288), 6, 2), ("cornell", {}, (40, 24), 8, 3)):
        gs = dev_scenes(name, **kw)
        sd = gs.desc
        cam = Camera.for_scene(sd, (w, h))
        f, b, rays = _oracle_frame(oracle, sd, w, h, abi.RT_RENDERER_WAVEFRONT, depth, spp, use_bvh=(name == "atrium"))
        for lanes in (1, 3):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            r = WavefrontRenderer(gs, (w, h), depth, spp)
            for k in env:
                monkeypatch.delenv(k)
            r.set_schedule(finish_depth=ALL_BOUNCES, fused_bounce=True, stream_lanes=lanes)
            got = r.render_frame(cam)
            assert got.kernels["wf_shoot"] == lanes * spp * depth and got.kernels["wf_finish"] == 0
            _assert_frames_equal(got.rgba_f32, got.rgba_u8, got.rays, f, b, rays, f"{name} SHOOT claims {env} on {lanes} lanes")
            r.close()


@pytest.mark.parametrize("finish_depth", [0, 1, 3, 7, 8, 99, ALL_BOUNCES])
def test_wavefront_finish_depth_keeps_the_frame(gpu_scenes, oracle, finish_depth):
    """The wavefront renderer's schedule: the first rt_schedule.finish_depth bounces launch by launch (EXTEND + SHADE with global
    compaction, as the reference's shoot_rays per bounce), then k_wf_finish follows the surviving rays to the end of their paths in
    one launch per sample. Every split — 0 (all in k_wf_finish), in between, >= max_depth (the reference's schedule) — must give the
    same frame, unorm8 image and ray count as the oracle's WavefrontRenderer, with and without Russian roulette, on full frames and
    odd tiles."""
    for name, kw, (w, h), depth, spp in (("cornell", {}, (96, 64), 8, 4), ("atrium", {"detail": 1}, (192, 108), 10, 3)):
        gs = gpu_scenes(name, **kw)
        sd = gs.desc
        cam = Camera.for_scene(sd, (w, h))
        use_bvh = name != "cornell"
        r = WavefrontRenderer(gs, (w, h), depth, spp)
        r.set_schedule(finish_depth=finish_depth)
        got = r.render_frame(cam)
        d0 = min(finish_depth, depth)
        lanes = 1 if finish_depth == 0 else PER_BOUNCE_LANES if finish_depth >= depth else 2
        assert got.hw_queues == HW_QUEUES
        assert got.finish_depth == d0 and got.stream_lanes == lanes
        assert got.kernels["wf_extend"] == got.kernels["wf_shade"] == lanes * spp * d0
        assert got.kernels["wf_finish"] == (0 if d0 == depth else lanes * (spp if d0 else 1))
        f, b, rays = _oracle_frame(oracle, sd, w, h, abi.RT_RENDERER_WAVEFRONT, depth, spp, use_bvh=use_bvh)
        _assert_frames_equal(got.rgba_f32, got.rgba_u8, got.rays, f, b, rays, f"{name} finish_depth={finish_depth}")
        r.set_russian_roulette(2)
        got_rr = r.render_frame(cam)
        f, b, rays = _oracle_frame(oracle, sd, w, h, abi.RT_RENDERER_WAVEFRONT, depth, spp, use_bvh=use_bvh, rr_start=2)
        _assert_frames_equal(got_rr.rgba_f32, got_rr.rgba_u8, got_rr.rays, f, b, rays, f"{name} finish_depth={finish_depth} rr")
        r.set_russian_roulette(0)
        r.set_tile(2, 5, 8)
        tile = r.render_frame(cam)
        f, b, rays = _oracle_frame(oracle, sd, w, h, abi.RT_RENDERER_WAVEFRONT, depth, spp, use_bvh=use_bvh, rank=2, world=5, strip_rows=8)
        _assert_frames_equal(tile.rgba_f32, tile.rgba_u8, tile.rays, f, b, rays, f"{name} finish_depth={finish_depth} tile 2/5")
        r.close()
    # max_depth 1: k_wf_finish (if it runs at all) only sees the last bounce
    gs = gpu_scenes("cube")
    sd = gs.desc
    r = WavefrontRenderer(gs, (64, 40), 1, 3)
    r.set_schedule(finish_depth=finish_depth)
    got = r.render_frame(Camera.for_scene(sd, (64, 40)))
    f, b, rays = _oracle_frame(oracle, sd, 64, 40, abi.RT_RENDERER_WAVEFRONT, 1, 3)
    _assert_frames_equal(got.rgba_f32, got.rgba_u8, got.rays, f, b, rays, "depth 1")
    r.close()


@pytest.mark.parametrize("reorder,matsort", [(1, 0), (0, 1), (1, 1)])
def test_wavefront_reordering_keeps_the_frame(gpu_scenes, oracle, reorder, matsort):
    """SURVEY §8f row f-3, ray re-ordering between bounces (rt_schedule.reorder: the compaction bins survivors by direction octant and
    4x4x4 origin cell; rt_schedule.matsort: SHADE partitions its rays by material kind). Both act in k_wf_shade, i.e. in the PER-BOUNCE
    schedule (finish_depth = all bounces: EXTEND + SHADE launch pairs with compaction in between, the reference's shape,
    src/render_wavefront.cpp:282-311) — which the test selects and then ASSERTS ran, from the launch counts the library reports: the
    re-ordering variants of k_wf_shade were launched once per sample, bounce and stream lane. The queue order is not part of the result,
    so frame, unorm8 image and ray count stay bit-identical to the oracle's — on both scenes, with Russian roulette (whose extra RNG
    draw sits between shading and compaction) and on an odd tile (short queues, blocks that are not full)."""
    for name, kw, (w, h), depth, spp in (("cornell", {}, (96, 64), 8, 4), ("atrium", {"detail": 1}, (256, 144), 10, 3)):
        gs = gpu_scenes(name, **kw)
        sd = gs.desc
        cam = Camera.for_scene(sd, (w, h))
        use_bvh = name == "atrium"
        r = WavefrontRenderer(gs, (w, h), depth, spp)
        r.set_schedule(finish_depth=ALL_BOUNCES, reorder=reorder, matsort=matsort)
        got = r.render_frame(cam)
        pairs = got.stream_lanes * spp * depth
        assert got.finish_depth == depth and got.kernels["wf_finish"] == 0, got.kernels
        assert got.kernels["wf_extend"] == got.kernels["wf_shade"] == pairs
        assert got.kernels["wf_shade_reorder"] == (pairs if reorder else 0) and got.kernels["wf_shade_matsort"] == (pairs if matsort else 0)
        f, b, rays = _oracle_frame(oracle, sd, w, h, abi.RT_RENDERER_WAVEFRONT, depth, spp, use_bvh=use_bvh)
        _assert_frames_equal(got.rgba_f32, got.rgba_u8, got.rays, f, b, rays, f"{name} reorder={reorder} matsort={matsort}")
        r.set_tile(1, 3, 8)
        tile = r.render_frame(cam)
        assert tile.kernels["wf_shade_reorder"] == (tile.stream_lanes * spp * depth if reorder else 0)
        ft, bt, rt_ = _oracle_frame(oracle, sd, w, h, abi.RT_RENDERER_WAVEFRONT, depth, spp, use_bvh=use_bvh, rank=1, world=3, strip_rows=8)
        _assert_frames_equal(tile.rgba_f32, tile.rgba_u8, tile.rays, ft, bt, rt_, f"{name} re-ordered tile 1/3")
        r.set_tile(0, 1, 8)
        r.set_russian_roulette(2)
        got_rr = r.render_frame(cam)
        assert got_rr.kernels["wf_shade_matsort"] == (pairs if matsort else 0)
        f, b, rays = _oracle_frame(oracle, sd, w, h, abi.RT_RENDERER_WAVEFRONT, depth, spp, use_bvh=use_bvh, rr_start=2)
        _assert_frames_equal(got_rr.rgba_f32, got_rr.rgba_u8, got_rr.rays, f, b, rays, f"{name} re-ordered, roulette")
        r.close()


@pytest.mark.parametrize("w,h,ordered", [(256, 144, True), (250, 144, False), (256, 140, False)])
def test_cost_ordered_second_launch_keeps_the_frame(gpu_scenes, oracle, w, h, ordered):
    """rt_schedule.cost_order = 1: sample 0 of every pixel in a launch of its own (recording what each path cost), the 8x8 blocks
    sorted by that cost (k_wf_tile_cost, k_wf_order_tiles), the remaining samples with the most expensive blocks first. Automatic
    selection only picks it for large frames at >= 32 spp; forced here on a small one, against cost_order = 0 and the oracle. A tile
    that does not consist of whole 8x8 blocks falls back to queue order (and the stats say that it did)."""
    for name, kw, depth, spp in (("cornell", {}, 8, 5), ("atrium", {"detail": 1}, 10, 3)):
        gs = gpu_scenes(name, **kw)
        sd = gs.desc
        cam = Camera.for_scene(sd, (w, h))
        r = WavefrontRenderer(gs, (w, h), depth, spp)
        r.set_schedule(cost_order=1)
        on = r.render_frame(cam)
        assert on.cost_ordered == ordered and on.kernels["wf_tile_order"] == (2 if ordered else 0)
        assert on.kernels["wf_finish"] == on.kernels["wf_generate"] == (2 if ordered else 1)
        r.set_schedule(cost_order=0)
        off = r.render_frame(cam)
        assert not off.cost_ordered and off.kernels["wf_finish"] == 1
        f, b, rays = _oracle_frame(oracle, sd, w, h, abi.RT_RENDERER_WAVEFRONT, depth, spp, use_bvh=(name == "atrium"))
        _assert_frames_equal(on.rgba_f32, on.rgba_u8, on.rays, f, b, rays, f"{name} cost-ordered")
        _assert_frames_equal(off.rgba_f32, off.rgba_u8, off.rays, f, b, rays, f"{name} queue order")
        if ordered:  # a tile of the split keeps whole blocks (8-row strips): ordered too
            r.set_schedule(cost_order=1)
            r.set_tile(1, 2, 8)
            t = r.render_frame(cam)
            assert t.cost_ordered
            ft, bt, rt_ = _oracle_frame(oracle, sd, w, h, abi.RT_RENDERER_WAVEFRONT, depth, spp, use_bvh=(name == "atrium"), rank=1, world=2, strip_rows=8)
            _assert_frames_equal(t.rgba_f32, t.rgba_u8, t.rays, ft, bt, rt_, f"{name} cost-ordered tile")
        r.close()


@pytest.mark.parametrize("cls,kind", KINDS)
def test_render_is_deterministic_and_reusable(gpu_scenes, cls, kind):
    gs = gpu_scenes("atrium", detail=1)
    w, h = 256, 144
    cam = Camera.for_scene(gs.desc, (w, h))
    r = cls(gs, (w, h), 10, 4)
    a, b = r.render_frame(cam), r.render_frame(cam)  # same renderer twice: state is re-initialised per frame
    assert a.rays == b.rays and a.rays > w * h * 4
    np.testing.assert_array_equal(a.rgba_f32, b.rgba_f32)
    np.testing.assert_array_equal(a.rgba_u8, np.clip(np.rint(np.clip(a.rgba_f32, 0, 1) * 255), 0, 255).astype(np.uint8))
    r.close()


def test_device_output_pointers(gpu_scenes):
    """rt_render_frame_device writes into caller-owned device memory (torch tensors as plain pointers)."""
    torch = pytest.importorskip("torch")
    gs = gpu_scenes("cube")
    w, h = 128, 72
    cam = Camera.for_scene(gs.desc, (w, h))
    r = WavefrontRenderer(gs, (w, h), 10, 2)
    host = r.render_frame(cam)
    f = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    b = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    fr = r.render_frame_device(cam, f.data_ptr(), b.data_ptr())
    torch.cuda.synchronize()
    assert fr.rays == host.rays
    np.testing.assert_array_equal(f.cpu().numpy(), host.rgba_f32)
    np.testing.assert_array_equal(b.cpu().numpy(), host.rgba_u8)
    r.close()


def test_edge_cases(gpu_scenes, oracle, scene_cache):
    # empty scene: every ray misses -> sky; max_depth 0: no rays at all, black frame
    gs = gpu_scenes("empty")
    cam = Camera((40, 24), (0, 0, 0), (0, 0, -1), 1.0)
    for cls, kind in KINDS:
        r = cls(gs, (40, 24), 10, 3)
        fr = r.render_frame(cam)
        assert fr.rays == 40 * 24 * 3
        f, b, rays = oracle.OracleScene(scene_cache("empty")).render(oracle.camera(40, 24, (0, 0, 0), (0, 0, -1), 1.0), kind, 10, 3)
        np.testing.assert_array_equal(fr.rgba_f32, f)
        r.close()
        r0 = cls(gpu_scenes("cube"), (40, 24), 0, 2)
        fr0 = r0.render_frame(Camera.for_scene(scene_cache("cube"), (40, 24)))
        assert fr0.rays == 0 and not fr0.rgba_f32[..., :3].any()
        r0.close()
    # 1x1 image and a size below one tile
    for (w, h) in ((1, 1), (3, 5)):
        gs = gpu_scenes("cube")
        sd = scene_cache("cube")
        for cls, kind in KINDS:
            r = cls(gs, (w, h), 5, 2)
            fr = r.render_frame(Camera.for_scene(sd, (w, h)))
            f, b, rays = oracle.OracleScene(sd).render(
                oracle.camera(w, h, sd.camera.position, sd.camera.direction, sd.camera.focal_length), kind, 5, 2)
            _assert_frames_equal(fr.rgba_f32, fr.rgba_u8, fr.rays, f, b, rays, f"{w}x{h}")
            r.close()
    # argument errors come back as codes, not crashes
    lib = abi.load_library()
    h_ = C.c_void_p()
    assert lib.rt_renderer_create(7, gpu_scenes("cube").h, 8, 8, 1, 1, 0, C.byref(h_)) == abi.RT_ERR_INVALID
    assert lib.rt_renderer_create(0, gpu_scenes("cube").h, 8, 8, 1, 0, 0, C.byref(h_)) == abi.RT_ERR_INVALID
    r = WavefrontRenderer(gpu_scenes("cube"), (8, 8), 1, 1)
    with pytest.raises(abi.RtError):
        r.render_frame(Camera((9, 8), (0, 0, 0), (0, 0, -1), 1.0))
    with pytest.raises(abi.RtError):
        r.set_tile(2, 2)
    r.close()


@pytest.mark.parametrize("cls,kind", KINDS)
def test_full_size_properties(gpu_scenes, oracle, scene_cache, cls, kind):
    """BASELINE config 4 at full resolution (1920x1080, reduced spp so the test stays short): checked
    through size-independent properties — (a) rows sampled across the frame equal the oracle's rows,
    rendered as 1-row... tiles of the same frame, (b) rays/path within [1, depth], (c) unorm8 == quantised
    fp32, (d) an 8-way tile split reassembles to the same frame."""
    sd = scene_cache("atrium", detail=4)
    gs = gpu_scenes("atrium", detail=4)
    w, h, spp, depth = 1920, 1080, 2, 10
    cam = Camera.for_scene(sd, (w, h))
    r = cls(gs, (w, h), depth, spp)
    full = r.render_frame(cam)
    assert w * h * spp <= full.rays <= w * h * spp * depth
    assert 4.0 < full.rays / (w * h * spp) < 10.0  # enclosed scene: long paths (Sponza ~9.2)
    np.testing.assert_array_equal(full.rgba_u8[..., :3],
                                  np.rint(np.clip(full.rgba_f32[..., :3], 0, 1) * 255).astype(np.uint8))
    assert np.isfinite(full.rgba_f32).all() and (full.rgba_f32[..., 3] == 1).all()
    # (d) tile split
    parts, rays = [], 0
    for rank in range(8):
        r.set_tile(rank, 8, 8)
        fr = r.render_frame(cam)
        parts.append(fr.rgba_f32)
        rays += fr.rays
    r.close()
    assert rays == full.rays
    np.testing.assert_array_equal(assemble_tiles(parts, h, 8, 8), full.rgba_f32)
    # (a) oracle spot check: strips 5, 60 and 130 of the frame (8 rows each) via the oracle's tile split
    osc = oracle.OracleScene(sd)
    ocam = oracle.camera(w, h, sd.camera.position, sd.camera.direction, sd.camera.focal_length)
    n_strips = (h + 7) // 8
    for strip in (5, 60, 130):
        f, b, _ = osc.render(ocam, kind, depth, spp, use_bvh=True, rank=strip, world=n_strips, strip_rows=8)
        got = full.rgba_f32[strip * 8: strip * 8 + 8]
        nbad = int((got != f).any(-1).sum())
        rmse = float(np.sqrt(np.mean((got.astype(np.float64) - f) ** 2)))
        assert nbad == 0, f"strip {strip}: {nbad} pixels differ from the oracle (rmse {rmse:.3e})"


def _assert_strips_equal_the_oracle(oracle, sd, kind, w, h, depth, spp, frames, strips, local_strip_of=lambda k: k, what=""):
    """Bit-exact comparison of 8-row strips of full-size GPU frames with the oracle. The oracle renders strip k alone as tile
    (rank k, world n_strips) of the same frame at the SAME spp and depth (a pixel's RNG stream runs through all its samples,
    so nothing can be reduced on one side only) — once; `frames` = [(label, rgba_f32, rgba_u8), ...] are all compared with it.
    `local_strip_of` maps a global strip index to its position in a frame."""
    osc = oracle.OracleScene(sd)
    ocam = oracle.camera(w, h, sd.camera.position, sd.camera.direction, sd.camera.focal_length)
    n_strips = (h + 7) // 8
    for k in strips:
        f, b, _ = osc.render(ocam, kind, depth, spp, use_bvh=True, rank=k, world=n_strips, strip_rows=8)
        lk = local_strip_of(k)
        for label, got_f32, got_u8 in frames:
            gf, gb = got_f32[lk * 8: lk * 8 + f.shape[0]], got_u8[lk * 8: lk * 8 + f.shape[0]]
            nbad = int((gf != f).any(-1).sum())
            rmse = float(np.sqrt(np.mean((gf.astype(np.float64) - f) ** 2)))
            assert nbad == 0, f"{what} [{label}] strip {k}: {nbad} pixels differ from the oracle (rmse {rmse:.3e}, tolerance {RMSE_TOL})"
            np.testing.assert_array_equal(gb, b)


# BASELINE.json configs 1-4 at their FULL sizes, both renderers where the config names both: size-independent properties
# (ray bounds, clamping, unorm8 == quantised fp32, idempotence, tile split) PLUS a bit-exact oracle comparison of the listed
# 8-row strips at the full spp and depth. Config 5 has its own test below.
FULL_CONFIGS = [
    ("triangle", {}, 256, 256, 1, 10, MegakernelRenderer, (0, 15, 31)),      # config 1
    ("cube", {}, 512, 512, 16, 10, WavefrontRenderer, (0, 30, 63)),          # config 2
    ("cornell", {}, 1024, 1024, 64, 10, WavefrontRenderer, (40, 100)),       # config 3
    ("cornell", {}, 1024, 1024, 64, 10, MegakernelRenderer, (40, 100)),      # config 3, other renderer
    ("atrium", {"detail": 4}, 1920, 1080, 64, 10, WavefrontRenderer, (7, 66, 134)),   # config 4 (the bench workload)
    ("atrium", {"detail": 4}, 1920, 1080, 64, 10, MegakernelRenderer, (7, 66, 134)),  # config 4, the bench's headline renderer
    # the reference's second benchmark scene class (benchmark.py:18, benchmark_avg.csv:20-21: minecraft.glb at depth 10, 128 spp) on the generated voxel terrain
    ("voxel", {"detail": 4}, 1920, 1080, 128, 10, WavefrontRenderer, (20, 70, 120)),
    ("voxel", {"detail": 4}, 1920, 1080, 128, 10, MegakernelRenderer, (20, 70, 120)),
]


@pytest.mark.parametrize("name,kw,w,h,spp,depth,cls,strips", FULL_CONFIGS)
def test_baseline_configs_at_full_size(gpu_scenes, scene_cache, oracle, name, kw, w, h, spp, depth, cls, strips):
    """... and for the wavefront renderer BOTH schedules at full size: the default (one k_wf_finish launch per frame) and the
    per-bounce pipeline (k_wf_extend + k_wf_shade with __ballot / mbcnt compaction between bounces, the reference's shape:
    src/render_wavefront.cpp:282-311) — asserted from the launch counts, whole frames bit-equal to each other, strips against the oracle."""
    sd = scene_cache(name, **kw)
    gs = gpu_scenes(name, **kw)
    kind = abi.RT_RENDERER_WAVEFRONT if cls is WavefrontRenderer else abi.RT_RENDERER_MEGAKERNEL
    r = cls(gs, (w, h), depth, spp)
    cam = Camera.for_scene(sd, (w, h))
    a = r.render_frame(cam)
    assert w * h * spp <= a.rays <= w * h * spp * depth
    assert np.isfinite(a.rgba_f32).all() and (a.rgba_f32[..., 3] == 1).all() and (a.rgba_f32[..., :3] >= 0).all()
    if cls is WavefrontRenderer:
        assert a.rgba_f32[..., :3].max() <= 1.0  # every sample is clamped to [0,1] before averaging
        assert a.kernels["wf_finish"] >= 1 and a.kernels["wf_extend"] == 0 and a.samples_per_launch == spp  # the default: one launch per frame
    else:
        assert a.kernels["megakernel"] == 1
    np.testing.assert_array_equal(a.rgba_u8[..., :3], np.rint(np.clip(a.rgba_f32[..., :3], 0, 1) * 255).astype(np.uint8))
    # idempotence: the same renderer object renders the same frame again (all per-frame state is re-initialised)
    b = r.render_frame(cam, want_u8=False)
    assert b.rays == a.rays
    np.testing.assert_array_equal(a.rgba_f32, b.rgba_f32)
    # a 2-way tile split reassembles to the same frame and the same ray count
    parts, rays = [], 0
    for rank in range(2):
        r.set_tile(rank, 2, 8)
        fr = r.render_frame(cam, want_u8=False)
        parts.append(fr.rgba_f32)
        rays += fr.rays
    assert rays == a.rays
    np.testing.assert_array_equal(assemble_tiles(parts, h, 2, 8), a.rgba_f32)
    frames = [("default schedule", a.rgba_f32, a.rgba_u8)]
    if cls is WavefrontRenderer:
        r.set_tile(0, 1, 8)
        r.set_schedule(finish_depth=ALL_BOUNCES)
        pb = r.render_frame(cam)
        assert pb.finish_depth == depth and pb.kernels["wf_finish"] == 0
        assert pb.kernels["wf_extend"] == pb.kernels["wf_shade"] == pb.stream_lanes * spp * depth
        assert pb.rays == a.rays
        np.testing.assert_array_equal(pb.rgba_f32, a.rgba_f32)
        np.testing.assert_array_equal(pb.rgba_u8, a.rgba_u8)
        frames.append(("per-bounce schedule", pb.rgba_f32, pb.rgba_u8))
        r.set_schedule(finish_depth=ALL_BOUNCES, fused_bounce=True)  # ... and as ONE kernel per bounce (intersect + shade + compact)
        fb = r.render_frame(cam)
        assert fb.kernels["wf_shoot"] == fb.stream_lanes * spp * depth and fb.kernels["wf_extend"] == fb.kernels["wf_finish"] == 0
        assert fb.rays == a.rays
        np.testing.assert_array_equal(fb.rgba_f32, a.rgba_f32)
        frames.append(("fused per-bounce schedule", fb.rgba_f32, fb.rgba_u8))
    r.close()
    _assert_strips_equal_the_oracle(oracle, sd, kind, w, h, depth, spp, frames, strips, what=f"{name} {w}x{h} {spp}spp {cls.__name__}")


@pytest.mark.parametrize("cls,kind", [(WavefrontRenderer, abi.RT_RENDERER_WAVEFRONT), (MegakernelRenderer, abi.RT_RENDERER_MEGAKERNEL)])
def test_config5_as_stated_tile_0_of_8(gpu_scenes, scene_cache, oracle, cls, kind):
    """BASELINE.json config 5 exactly as stated — atrium (detail 4, 283k triangles), 3840x2160, 256 spp, depth 16, the
    wavefront renderer with wave compaction (and the megakernel beside it), the tile ONE GPU of the 8-GPU split renders:
    rank 0 of world 8, 8-row strips (34 strips, 272 rows, 1.04 M pixels, ~3.1 G rays). "Wavefront w/ wave-compaction" is run in BOTH
    of its forms: the default schedule (k_wf_finish: idle lanes refilled by __ballot / mbcnt ranks from the queue) and the per-bounce
    pipeline (k_wf_extend + k_wf_shade, survivors compacted between bounces: 256 x 16 launch pairs per stream lane) — which kernels
    ran is asserted from the library's launch counts. Properties of the whole tile plus a bit-exact oracle comparison of two of its
    strips at the full 256 spp and depth 16 (nothing is reduced: ~70 M rays per strip, some tens of seconds on the host cores)."""
    sd = scene_cache("atrium", detail=4)
    gs = gpu_scenes("atrium", detail=4)
    w, h, spp, depth, world = 3840, 2160, 256, 16, 8
    r = cls(gs, (w, h), depth, spp)
    r.set_tile(0, world, 8)
    rows = r.global_rows()
    assert len(rows) == 272 and all((y // 8) % world == 0 for y in rows)
    cam = Camera.for_scene(sd, (w, h))
    a = r.render_frame(cam)
    n_px = len(rows) * w
    assert a.rgba_f32.shape == (272, w, 4)
    assert n_px * spp <= a.rays <= n_px * spp * depth
    assert 4.0 < a.rays / (n_px * spp) < 16.0  # enclosed scene: long paths
    assert np.isfinite(a.rgba_f32).all() and (a.rgba_f32[..., 3] == 1).all() and (a.rgba_f32[..., :3] >= 0).all()
    frames = [("default schedule", a.rgba_f32, a.rgba_u8)]
    if cls is WavefrontRenderer:
        assert a.rgba_f32[..., :3].max() <= 1.0
        assert a.kernels["wf_finish"] >= 1 and a.kernels["wf_extend"] == 0
        r.set_schedule(finish_depth=ALL_BOUNCES)
        pb = r.render_frame(cam)
        assert pb.kernels["wf_finish"] == 0 and pb.kernels["wf_extend"] == pb.kernels["wf_shade"] == pb.stream_lanes * spp * depth
        assert pb.rays == a.rays
        np.testing.assert_array_equal(pb.rgba_f32, a.rgba_f32)
        frames.append(("per-bounce schedule", pb.rgba_f32, pb.rgba_u8))
        r.set_schedule(finish_depth=ALL_BOUNCES, fused_bounce=True)
        fb = r.render_frame(cam)
        assert fb.kernels["wf_shoot"] == fb.stream_lanes * spp * depth and fb.kernels["wf_extend"] == fb.kernels["wf_finish"] == 0
        assert fb.rays == a.rays
        np.testing.assert_array_equal(fb.rgba_f32, a.rgba_f32)
        frames.append(("fused per-bounce schedule", fb.rgba_f32, fb.rgba_u8))
    r.close()
    np.testing.assert_array_equal(a.rgba_u8[..., :3], np.rint(np.clip(a.rgba_f32[..., :3], 0, 1) * 255).astype(np.uint8))
    # global strips 64 and 200 belong to rank 0 (64 % 8 == 200 % 8 == 0) and are its local strips 8 and 25
    _assert_strips_equal_the_oracle(oracle, sd, kind, w, h, depth, spp, frames, (64, 200), local_strip_of=lambda k: k // world,
                                    what=f"config 5 {cls.__name__}")


@pytest.mark.parametrize("bvh", [abi.RT_BVH_SAH, abi.RT_BVH_LBVH, abi.RT_BVH_LBVH_GPU])
def test_far_away_ray_origins_equal_brute_force(oracle, scene_cache, bvh):
    """Ray origins up to 100 scene extents away from the scene (inside the enforced range of the closest-hit contract: the padding of
    the boxes, 2e-5 x scene scale, covers fp32 rounding of the slab arithmetic for origins that far) on exact
    diagonals through the cube's corners and centre — equal slab distances on all three axes, the configuration in which an
    ABSENT child's inverted box (qlo = 255 > qhi = 0) is closest to testing as a hit: the inner step relies on the inversion alone
    and has no explicit kChildEmpty test, which is sound inside the contract's range — and on random far origins, against the CPU
    brute force. (Beyond the range the entry points refuse: test_contract_range_is_enforced.)"""
    sd = scene_cache("cube")
    gs, osc = Scene(sd, 0, bvh), oracle.OracleScene(sd)
    tw = sd.world_triangles().reshape(-1, 3)
    lo, hi = tw.min(0), tw.max(0)
    c, ext = (lo + hi) / 2, float((hi - lo).max())
    rng = np.random.default_rng(11)
    org, dirs = [], []
    for dist in (3.0, 30.0, 100.0):
        for sx in (-1, 1):
            for sy in (-1, 1):
                for sz in (-1, 1):
                    d = np.array([sx, sy, sz], np.float64)
                    for target in (c, lo, hi, c + 0.25 * ext * d):
                        org.append(target - d * dist * ext), dirs.append(d)
                        org.append(target - d * dist * ext), dirs.append(d * 1e-3)   # unnormalised, as the renderers store them
        t = rng.uniform(lo, hi, (200, 3))
        d = rng.normal(size=(200, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        org.extend(t - d * dist * ext), dirs.extend(d)
    org, dirs = np.asarray(org, np.float32), np.asarray(dirs, np.float32)
    gt, gu, gv, gtri = gs.intersect(org, dirs)
    et, eu, ev, etri = osc.intersect(org, dirs, use_bvh=False)
    np.testing.assert_array_equal(gtri, etri)
    np.testing.assert_array_equal(gt, et)
    np.testing.assert_array_equal(gu, eu)
    np.testing.assert_array_equal(gv, ev)
    assert (gtri != NO_TRI).sum() > 100
    gs.close()


def test_contract_range_is_enforced(gpu_scenes, oracle, scene_cache):
    """Both sides of the limit of the closest-hit contract (include/rt_mi355x.h: origins at most 100 scene scales outside the scene's
    bounds on any axis; src/trace_ray.hpp:18-27 states none, so the narrowing must not be silent). Just inside: answered, and equal
    to the brute force. Just outside, or not finite: RT_ERR_INVALID naming the ray — for rt_intersect_batch and, through the camera
    centre, for both renderers."""
    sd = scene_cache("cube")
    gs, osc = gpu_scenes("cube"), oracle.OracleScene(sd)
    info = gs.info()
    lo, hi = np.array(info.bounds_lo, np.float64), np.array(info.bounds_hi, np.float64)
    scale = max(float((hi - lo).max()), float(np.abs(np.concatenate([lo, hi])).max()))
    c = (lo + hi) / 2
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    inside = np.array([np.where(a > 0, hi, np.where(a < 0, lo, c)) + a * 99.5 * scale for a in axes], np.float32)
    outside = np.array([np.where(a > 0, hi, np.where(a < 0, lo, c)) + a * 100.5 * scale for a in axes], np.float32)
    dirs = (-axes).astype(np.float32)  # straight back at the cube
    g = gs.intersect(inside, dirs)
    e = osc.intersect(inside, dirs, use_bvh=False)
    for x, y in zip(g, e):
        np.testing.assert_array_equal(x, y)
    assert (g[3] != NO_TRI).all()
    for k in range(6):
        org = inside.copy()
        org[k] = outside[k]
        with pytest.raises(abi.RtError, match=f"ray {k}: origin more than 100 scene scales"):
            gs.intersect(org, dirs)
    bad = inside.copy()
    bad[2, 1] = np.nan
    with pytest.raises(abi.RtError, match="ray 2"):
        gs.intersect(bad, dirs)
    w, h = 32, 24
    for cls, kind in KINDS:
        r = cls(gs, (w, h), 4, 2)
        near = r.render_frame(Camera((w, h), tuple(inside[2]), tuple(dirs[2]), 200.0))  # +z side, looking back: a narrow view of the cube
        ocam = oracle.camera(w, h, tuple(inside[2]), tuple(dirs[2]), 200.0)
        f, b, rays = osc.render(ocam, kind, 4, 2, use_bvh=False)
        _assert_frames_equal(near.rgba_f32, near.rgba_u8, near.rays, f, b, rays, f"camera at 99.5 scales {cls.__name__}")
        assert rays > w * h * 2  # it does see the cube
        with pytest.raises(abi.RtError, match="camera lies more than 100 scene scales"):
            r.render_frame(Camera((w, h), tuple(outside[2]), tuple(dirs[2]), 200.0))
        again = r.render_frame(Camera((w, h), tuple(inside[2]), tuple(dirs[2]), 200.0))  # the refusal leaves the renderer usable
        assert again.rays == rays
        r.close()


def test_gather_overlaps_with_the_next_frame(gpu_scenes, oracle):
    """rt_frame_gather_begin / rt_comm_wait: the gather of frame N is only ENQUEUED (event waits between the renderers' streams and the
    root's, no host wait), frame N+1 is begun on every renderer right behind it, and frame N is collected afterwards — every frame that
    comes back is the single-device frame, for a moving camera (so that a frame overwritten too early would show), on the RCCL path
    (one rank) and on the device-copy path (three tiles on one device)."""
    gs = gpu_scenes("cornell")
    sd = gs.desc
    w, h, depth, spp = 120, 93, 5, 2
    poses = [tuple(np.asarray(sd.camera.position) + np.array([0.15 * i, -0.05 * i, 0.1 * i])) for i in range(4)]
    cams = [Camera((w, h), p, sd.camera.direction, sd.camera.focal_length) for p in poses]
    ref = WavefrontRenderer(gs, (w, h), depth, spp)
    want = [ref.render_frame(c) for c in cams]
    ref.close()
    assert not np.array_equal(want[0].rgba_f32, want[1].rgba_f32)
    for devices in ((0,), (0, 0, 0)):
        comm = TileComm(devices)
        n = len(devices)
        assert comm.size == n
        rs = []
        for k in range(n):
            r = WavefrontRenderer(gs, (w, h), depth, spp)
            r.set_tile(k, n, 8)
            rs.append(r)
        lib = abi.load_library()

        def begin(cam):
            for r in rs:
                r.begin_frame(cam, d_f32=lib.rt_renderer_tile_f32(r.h), d_u8=lib.rt_renderer_tile_u8(r.h))

        begin(cams[0])
        for i in range(len(cams)):
            rays = sum(r.end_frame().rays for r in rs)
            comm.gather_begin(rs)
            if i + 1 < len(cams):
                begin(cams[i + 1])  # in flight while frame i is gathered and copied out
            f, b = comm.wait((h, w))
            assert rays == want[i].rays
            np.testing.assert_array_equal(f, want[i].rgba_f32)
            np.testing.assert_array_equal(b, want[i].rgba_u8)
        comm.gather_begin(rs, want_f32=False)  # only the u8 plane this time: asking rt_comm_wait for the other one is an error, not stale data
        with pytest.raises(abi.RtError, match="not gathered"):
            comm.wait((h, w), want_f32=True, want_u8=True)
        _, b = comm.wait((h, w), want_f32=False)
        np.testing.assert_array_equal(b, want[-1].rgba_u8)
        for r in rs:
            r.close()
        comm.close()


def _soup_scene(rng, n_tris, scale=1.0, offset=(0, 0, 0), duplicates=0, degenerate=0, n_inst=3):
    """Random triangle soup spread over several rotated/scaled instances, with exact duplicate triangles (equal t:
    the lowest global index must win) and zero-area triangles (must never be hit)."""
    sb = scenes.SceneBuilder("soup")
    mats = [sb.add_material(scenes.Material(abi.RT_MAT_DIFFUSE, (0.5, 0.5, 0.5))),
            sb.add_material(scenes.Material(abi.RT_MAT_METALLIC, (0.9, 0.9, 0.9), roughness=0.3)),
            sb.add_material(scenes.Material(abi.RT_MAT_DIELECTRIC, ior=1.4))]
    for i in range(n_inst):
        m = n_tris // n_inst
        c = rng.uniform(-1, 1, (m, 1, 3))
        p = (c + rng.normal(size=(m, 3, 3)) * rng.uniform(0.01, 0.4, (m, 1, 1))).astype(np.float32)
        if duplicates:
            p[-duplicates:] = p[:duplicates]            # exact copies later in the index order
        if degenerate:
            p[1:1 + degenerate, 2] = p[1:1 + degenerate, 1]  # two identical vertices: zero area
        pos = (p.reshape(-1, 3) * scale).astype(np.float32)
        nrm = rng.normal(size=pos.shape).astype(np.float32)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        uv = rng.uniform(0, 1, (pos.shape[0], 2)).astype(np.float32)
        idx = np.arange(pos.shape[0], dtype=np.uint32).reshape(-1, 3)
        xf = scenes.trs(tuple(np.asarray(offset, np.float64) + rng.uniform(-0.5, 0.5, 3) * scale),
                        scenes.quat_axis_angle(rng.normal(size=3), rng.uniform(0, 3)), tuple(rng.uniform(0.5, 1.5, 3)))
        sb.add_instance(sb.add_mesh(pos, nrm, uv, idx), mats[i % 3], xf)
    return sb.build()


@pytest.mark.parametrize("seed,n_tris,scale,offset", [(1, 300, 1.0, (0, 0, 0)), (2, 2400, 1.0, (0, 0, 0)),
                                                       (3, 600, 1e-3, (0, 0, 0)), (4, 600, 250.0, (1000.0, -2000.0, 500.0)),
                                                       (5, 9, 1.0, (0, 0, 0))])
@pytest.mark.parametrize("bvh", [abi.RT_BVH_SAH, abi.RT_BVH_LBVH_GPU])
def test_random_soups_intersect_and_render_equal_the_oracle(oracle, seed, n_tris, scale, offset, bvh):
    """Edge cases of the intersection contract on random instanced triangle soups: duplicate coplanar triangles (tie ->
    lowest global index), zero-area triangles, tiny (1e-3) and huge far-from-origin (1e3) coordinates, all three
    materials with arbitrary normals; checked for batch queries and for whole renders, brute force on the CPU."""
    rng = np.random.default_rng(seed)
    sd = _soup_scene(rng, n_tris, scale, offset, duplicates=min(20, n_tris // 9), degenerate=min(5, n_tris // 9))
    sd.camera = scenes.CameraPose(tuple(np.asarray(offset, np.float64) + np.array([0.0, 0.0, 3.0]) * scale), (0.0, 0.0, -1.0), 1.5)
    gs, osc = Scene(sd, 0, bvh), oracle.OracleScene(sd)
    gs.check_bvh()
    tw = sd.world_triangles().reshape(-1, 3)
    lo, hi = tw.min(0), tw.max(0)
    n = 20000
    org = rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), (n, 3)).astype(np.float32)
    dirs = (rng.normal(size=(n, 3)) * rng.uniform(0.01, 2.0, (n, 1))).astype(np.float16).astype(np.float32)
    g, e = gs.intersect(org, dirs), osc.intersect(org, dirs, use_bvh=False)
    for a, b in zip(g, e):
        np.testing.assert_array_equal(a, b)
    hit = e[3] != NO_TRI
    assert hit.sum() > 100
    w, h = 64, 48
    ocam = oracle.camera(w, h, sd.camera.position, sd.camera.direction, sd.camera.focal_length)
    for cls, kind in KINDS:
        r = cls(gs, (w, h), 8, 3)
        fr = r.render_frame(Camera.for_scene(sd, (w, h)))
        f, b, rays = osc.render(ocam, kind, 8, 3, use_bvh=False)
        # random normals make NaN-free shading unlikely to matter, but compare NaN-aware to be safe
        assert fr.rays == rays
        np.testing.assert_array_equal(np.nan_to_num(fr.rgba_f32, nan=-1.0), np.nan_to_num(f, nan=-1.0))
        r.close()
    gs.close()


@pytest.mark.parametrize("rr", [1, 3, 9, 10])
def test_russian_roulette_extension_equals_the_oracle(oracle, scene_cache, rr):
    """The optional Russian roulette (rt_renderer_set_russian_roulette; a to-do upstream) follows one rule on the GPU
    and in the oracle: still bit-exact, in both renderers, and switching it off restores the reference's image."""
    sd = scene_cache("atrium", detail=1)
    gs, osc = Scene(sd, 0), oracle.OracleScene(sd)
    w, h = 96, 54
    ocam, cam = oracle.camera(w, h, sd.camera.position, sd.camera.direction, sd.camera.focal_length), Camera.for_scene(sd, (w, h))
    for cls, kind in KINDS:
        r = cls(gs, (w, h), 10, 6)
        base = r.render_frame(cam)
        r.set_russian_roulette(rr)
        fr = r.render_frame(cam)
        f, b, rays = osc.render(ocam, kind, 10, 6, rr_start=rr)
        assert fr.rays == rays
        np.testing.assert_array_equal(fr.rgba_f32, f)
        np.testing.assert_array_equal(fr.rgba_u8, b)
        assert (rays < base.rays) == (rr < 10)
        r.set_russian_roulette(0)
        again = r.render_frame(cam)
        assert again.rays == base.rays
        np.testing.assert_array_equal(again.rgba_f32, base.rgba_f32)
        r.close()
    gs.close()


def test_wavefront_frame_replayed_as_a_hip_graph_is_identical(oracle, scene_cache):
    """rt_schedule.hip_graph captures the frame's launch sequence (both streams) into a hipGraph and replays it per frame: same
    image and ray count, also after the camera moves (the camera is the graph's only per-frame input)."""
    sd = scene_cache("cornell")
    gs, osc = Scene(sd, 0), oracle.OracleScene(sd)
    w, h = 80, 64
    r = WavefrontRenderer(gs, (w, h), 6, 5)
    r.set_schedule(hip_graph=True)
    for pos in (sd.camera.position, tuple(np.asarray(sd.camera.position) + np.array([0.2, -0.1, 0.3])), sd.camera.position):
        cam = Camera((w, h), pos, sd.camera.direction, sd.camera.focal_length)
        fr = r.render_frame(cam)
        f, b, rays = osc.render(oracle.camera(w, h, pos, sd.camera.direction, sd.camera.focal_length), abi.RT_RENDERER_WAVEFRONT, 6, 5)
        assert fr.rays == rays
        np.testing.assert_array_equal(fr.rgba_f32, f)
        np.testing.assert_array_equal(fr.rgba_u8, b)
    r.close()
    gs.close()


def test_every_texel_value_shades_identically(oracle):
    """A camera-facing quad with a texture that holds every byte value in every channel, lit by the sky only: each pixel
    is albedo(texel) x sky after one diffuse bounce, so any difference in the texel -> float conversion would show."""
    sb = scenes.SceneBuilder("texels")
    iu, iv = np.meshgrid(np.arange(512), np.arange(512), indexing="xy")
    tex = np.stack([iu % 256, iv % 256, (iu // 2 + iv // 2) % 256, np.full_like(iu, 255)], -1).astype(np.uint8)
    layer = sb.add_texture(tex)
    mat = sb.add_material(scenes.Material(abi.RT_MAT_DIFFUSE, (1.0, 1.0, 1.0), layer))
    sb.add_instance(sb.add_mesh(*scenes.mesh_quad((-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0), nx=1, ny=1)), mat)
    sb.sky = np.array([1.0, 0.75, 0.5], np.float32)
    sb.camera = scenes.CameraPose((0.0, 0.0, 2.0), (0.0, 0.0, -1.0), 2.0)
    sd = sb.build()
    gs, osc = Scene(sd, 0), oracle.OracleScene(sd)
    w = h = 512
    ocam = oracle.camera(w, h, sd.camera.position, sd.camera.direction, sd.camera.focal_length)
    for cls, kind in KINDS:
        r = cls(gs, (w, h), 2, 2)
        fr = r.render_frame(Camera.for_scene(sd, (w, h)))
        f, b, rays = osc.render(ocam, kind, 2, 2, use_bvh=False)
        assert fr.rays == rays
        np.testing.assert_array_equal(fr.rgba_f32, f)
        assert len(np.unique(np.round(fr.rgba_f32[..., 0] ** 2 * 255 * 2).astype(int))) > 200  # many distinct albedos were seen
        r.close()
    gs.close()


@pytest.mark.parametrize("cls,kind", KINDS)
def test_frames_of_two_renderers_in_flight_at_once(oracle, scene_cache, cls, kind):
    """rt_render_frame_begin / _end: two renderers (double buffering) keep a frame each in flight; every frame is the
    frame the blocking call renders, in any interleaving, and misuse is an error rather than a hang."""
    import torch
    sd = scene_cache("cornell")
    gs = Scene(sd, 0)
    w, h = 128, 96
    cam = Camera.for_scene(sd, (w, h))
    a, b = cls(gs, (w, h), 6, 4), cls(gs, (w, h), 6, 4)
    ref = a.render_frame(cam)
    bufs = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    rs = [a, b]
    pending = None
    for i in range(6):
        r = rs[i % 2]
        bufs[i % 2].zero_()
        torch.cuda.synchronize()
        r.begin_frame(cam, d_f32=bufs[i % 2].data_ptr())
        if pending is not None:
            fr = rs[pending].end_frame()
            assert fr.rays == ref.rays
            np.testing.assert_array_equal(bufs[pending].cpu().numpy(), ref.rgba_f32)
        pending = i % 2
    with pytest.raises(RuntimeError, match="not been collected"):
        rs[pending].begin_frame(cam, d_f32=bufs[pending].data_ptr())
    fr = rs[pending].end_frame()
    assert fr.rays == ref.rays
    np.testing.assert_array_equal(bufs[pending].cpu().numpy(), ref.rgba_f32)
    with pytest.raises(RuntimeError, match="no frame in flight"):
        a.end_frame()
    a.close(), b.close(), gs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bvh", [abi.RT_BVH_SAH, abi.RT_BVH_LBVH, abi.RT_BVH_LBVH_GPU])
def test_deep_traversal_stacks_spill_and_equal_the_oracle(oracle, bvh):
    """A pile of 8,192 large parallel triangles with one bounding box. All but two of them leave the corner free through which the
    rays pass, so a ray that looks down the pile enters EVERY child box of every node on its first descent and meets nothing: its stack
    grows by up to three entries per level — past the 11 usable LDS entries into the scratch spill (rt_device.h: stk_push / trav_pop,
    the sentinel in entry 0) — and the triangle it does hit (the sixth from either end) sits in a NEAR sibling, i.e. behind an entry that
    went through the spill. Batch queries and renders against brute force."""
    n = 8192
    z = -np.arange(n, dtype=np.float32) / np.float32(n)
    pos = np.zeros((n, 3, 3), np.float32)
    pos[:, 0] = (5.0, -5.0, 0.0)   # the hypotenuse: the same for both kinds
    pos[:, 1] = (-5.0, 7.0, 0.0)
    pos[:, 2] = (-5.0, -5.0, 0.0)  # kind B: covers 12 x + 10 y < 10, NOT the rays' corner (x, y in 1.5 .. 3)
    pos[[5, n - 6], 2] = (5.0, 7.0, 0.0)  # kind A: the other half of the same box
    pos[:, :, 2] = z[:, None]
    sb = scenes.SceneBuilder("pile")
    mat = sb.add_material(scenes.Material(abi.RT_MAT_DIFFUSE, (0.7, 0.6, 0.5)))
    p = pos.reshape(-1, 3)
    nrm = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (p.shape[0], 1))
    uv = np.zeros((p.shape[0], 2), np.float32)
    sb.add_instance(sb.add_mesh(p, nrm, uv, np.arange(p.shape[0], dtype=np.uint32).reshape(-1, 3)), mat, scenes.trs((0, 0, 0), (0, 0, 0, 1), (1, 1, 1)))
    sd = sb.build()
    sd.camera = scenes.CameraPose((2.25, 2.25, 3.0), (0.0, 0.0, -1.0), 6.0)  # a narrow view down the free corner
    gs, osc = Scene(sd, 0, bvh), oracle.OracleScene(sd)
    gs.check_bvh()
    assert gs.info().max_depth >= 6  # 3 pushes per level on the first descent: more than the LDS part of the stack holds
    rng = np.random.default_rng(11)
    m = 4096
    org = np.stack([rng.uniform(1.5, 3.0, m), rng.uniform(1.5, 3.0, m), rng.uniform(0.5, 3.0, m)], -1).astype(np.float32)
    org[m // 2:, 2] = rng.uniform(-3.0, -1.5, m - m // 2).astype(np.float32)  # half of them from below the pile, looking up
    dirs = np.stack([rng.normal(0, 0.02, m), rng.normal(0, 0.02, m), np.where(org[:, 2] > 0, -1.0, 1.0)], -1).astype(np.float16).astype(np.float32)
    g, e = gs.intersect(org, dirs), osc.intersect(org, dirs, use_bvh=False)
    for a, b in zip(g, e):
        np.testing.assert_array_equal(a, b)
    assert (e[3] != NO_TRI).sum() > m * 0.9 and set(np.unique(e[3][e[3] != NO_TRI])) == {5, n - 6}
    w, h = 64, 48
    ocam = oracle.camera(w, h, sd.camera.position, sd.camera.direction, sd.camera.focal_length)
    for cls, kind in KINDS:
        r = cls(gs, (w, h), 4, 2)
        fr = r.render_frame(Camera.for_scene(sd, (w, h)))
        f, b, rays = osc.render(ocam, kind, 4, 2, use_bvh=False)
        _assert_frames_equal(fr.rgba_f32, fr.rgba_u8, fr.rays, f, b, rays, f"pile {kind}")
        r.close()
    gs.close()


@pytest.mark.gpu
def test_instrumented_kernels_render_the_same_frame(gpu_scenes, oracle, monkeypatch, capfd):
    """RT_KERNEL_STATS=1 selects the STATS instantiations of the traversal kernels (wave-level step counters, scripts/final_profile.sh
    stats): separate kernels compiled from the same source, so they are held to the same frame — megakernel, the wavefront renderer's
    one-launch schedule, its per-bounce pair, the fused per-bounce kernel and the dynamic-queue instantiation — and must print their report."""
    gs = gpu_scenes("cornell")
    sd = gs.desc
    w, h, depth, spp = 96, 64, 6, 4
    cam = Camera.for_scene(sd, (w, h))
    monkeypatch.setenv("RT_KERNEL_STATS", "1")
    for cls, kind, sched in [(MegakernelRenderer, abi.RT_RENDERER_MEGAKERNEL, None), (WavefrontRenderer, abi.RT_RENDERER_WAVEFRONT, None),
                             (WavefrontRenderer, abi.RT_RENDERER_WAVEFRONT, dict(finish_depth=ALL_BOUNCES, fused_bounce=0)),
                             (WavefrontRenderer, abi.RT_RENDERER_WAVEFRONT, dict(finish_depth=ALL_BOUNCES, fused_bounce=1)),
                             (WavefrontRenderer, abi.RT_RENDERER_WAVEFRONT, dict(samples_per_launch=2, requeue=1))]:  # k_wf_finish<STATS, REQ>: the dynamic queue
        f, b, rays = _oracle_frame(oracle, sd, w, h, kind, depth, spp)
        r = cls(gs, (w, h), depth, spp)
        if sched:
            r.set_schedule(**sched)
        got = r.render_frame(cam)
        _assert_frames_equal(got.rgba_f32, got.rgba_u8, got.rays, f, b, rays, f"stats {cls.__name__} {sched}")
        r.close()
    assert "[rt stats]" in capfd.readouterr().err
    monkeypatch.setenv("RT_KERNEL_STATS", "2")  # the megakernel's timing-only instantiation (cycles per step / per shading round close to the product's)
    f, b, rays = _oracle_frame(oracle, sd, w, h, abi.RT_RENDERER_MEGAKERNEL, depth, spp)
    for slices in (0, 3):
        r = MegakernelRenderer(gs, (w, h), depth, spp)
        r.set_schedule(pixel_slices=slices)
        got = r.render_frame(cam)
        _assert_frames_equal(got.rgba_f32, got.rgba_u8, got.rays, f, b, rays, f"timing-only megakernel, slices {slices}")
        r.close()
    assert "timing-only instantiation" in capfd.readouterr().err


# ---- pixel slices of the megakernel (rt_schedule::pixel_slices) ------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,w,h,spp,depth", [("cornell", {}, 96, 64, 8, 6), ("atrium", {"detail": 1}, 120, 72, 5, 10), ("cube", {}, 97, 61, 3, 4),
                                                   ("cornell", {}, 48, 40, 67, 4)])  # (67 samples: slices end at multiples of TWO samples, the last unit is a short one)
@pytest.mark.parametrize("slices", [2, 3, 8])
@pytest.mark.parametrize("cls,kind", KINDS)
def test_pixel_slices_keep_the_frame_where_every_slice_has_to_wait(gpu_scenes, oracle, scene_cache, cls, kind, name, kw, w, h, spp, depth, slices):
    """A pixel's samples rendered as `slices` slices by different lanes (state through memory) instead of by one lane. On a tile this small
    every lane of the machine is free when the cursor hands out slice j of a pixel, so slice j is taken while slice j - 1 is still being
    rendered: the path where a lane WAITS for its pixel's state runs for every pixel. Same frame, same ray count, bit for bit; more slices
    than samples are cut down to one sample per slice."""
    sd = scene_cache(name, **kw)
    gs = gpu_scenes(name, **kw)
    f, b, rays = _oracle_frame(oracle, sd, w, h, kind, depth, spp)
    r = cls(gs, (w, h), depth, spp)  # (the wavefront renderer's one-launch schedule slices the same way: k_wf_finish<.., SLICED>)
    r.set_schedule(pixel_slices=slices)
    cam = Camera.for_scene(sd, (w, h))
    for frame in range(3):  # the state buffer is never cleared: tags tell the frames apart
        got = r.render_frame(cam)
        assert got.pixel_slices == min(slices, spp)
        _assert_frames_equal(got.rgba_f32, got.rgba_u8, got.rays, f, b, rays, f"{name} {slices} slices, frame {frame}")
    r.set_schedule(pixel_slices=0)
    got = r.render_frame(cam)
    assert got.pixel_slices == 1
    _assert_frames_equal(got.rgba_f32, got.rgba_u8, got.rays, f, b, rays, f"{name} unsliced")
    r.close()


def _slice_units(spp):
    """Units of samples a slice is made of (csrc/rt_frame.hip: slice_plan): forced slices are cut down to one unit each."""
    shift = 0
    while (spp - 1) >> shift >= 64:
        shift += 1
    return -(-spp // (1 << shift))


SLICE_FRAME_LIMIT_S = 5.0  # a lost hand-over waits ~15 s (kSliceWaitCap) before the frame fails: a slow frame is a failure, not a slow pass


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1, 1), (3, 5), (8, 4), (7, 9), (8, 8), (13, 5), (11, 12)])  # 1 ... 132 pixels: tiles below, at and above a wave
@pytest.mark.parametrize("spp", [4, 67, 130])  # slices end at multiples of 1, 2 (a short last unit) and 4 samples
@pytest.mark.parametrize("cls,kind", KINDS)
def test_pixel_slices_on_tiles_smaller_than_a_wave(gpu_scenes, oracle, scene_cache, cls, kind, w, h, spp):
    """Forced slices on tiles of fewer pixels than a wave has lanes. The wavefront renderer's cursor has as many slots per slice as the tile has
    pixels, and a wave's claim of up to 64 idle lanes once crossed two slice boundaries of such a tile: lanes then mapped to slots past the
    queue and the frame's later slices were never handed out (csrc/rt_launch.h: SliceCursor caps the claim). Three frames in a row each, as tags
    tell frames apart; every frame bit-exact and well inside the wait cap."""
    sd = scene_cache("cornell")
    gs = gpu_scenes("cornell")
    depth = 5
    f, b, rays = _oracle_frame(oracle, sd, w, h, kind, depth, spp)
    cam = Camera.for_scene(sd, (w, h))
    r = cls(gs, (w, h), depth, spp)
    for slices in (2, 3, 4, 8):
        r.set_schedule(pixel_slices=slices)
        for frame in range(3):
            t0 = time.perf_counter()
            got = r.render_frame(cam)
            dt = time.perf_counter() - t0
            what = f"{cls.__name__} {w}x{h} {spp} spp, {slices} slices, frame {frame}"
            assert dt < SLICE_FRAME_LIMIT_S, f"{what}: {dt:.1f} s"
            assert got.pixel_slices == min(slices, _slice_units(spp)), what
            _assert_frames_equal(got.rgba_f32, got.rgba_u8, got.rays, f, b, rays, what)
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,world,strip", [(5, 40, 8, 8),   # five tiles of 40 pixels; ranks 5 .. 7 have no rows
                                             (24, 20, 3, 8),  # the last rank has 4 rows
                                             (7, 9, 3, 8)])   # 56 pixels, 7 pixels, no rows
@pytest.mark.parametrize("cls,kind", KINDS)
def test_pixel_slices_on_split_tiles(gpu_scenes, oracle, scene_cache, cls, kind, w, h, world, strip):
    """Sliced tiles of a split frame, some below 64 pixels and some empty: assembled, they are the oracle's frame and each is its own
    renderer's unsliced tile; an empty tile renders without error and reports one slice."""
    sd = scene_cache("cornell")
    gs = gpu_scenes("cornell")
    depth, spp = 5, 67
    f, b, rays = _oracle_frame(oracle, sd, w, h, kind, depth, spp)
    cam = Camera.for_scene(sd, (w, h))
    r = cls(gs, (w, h), depth, spp)
    for slices in (2, 8):
        parts_f, parts_b, total = [], [], 0
        for rank in range(world):
            r.set_tile(rank, world, strip)
            rows = r.global_rows()
            assert all((y // strip) % world == rank for y in rows) and len(rows) == r.local_rows
            r.set_schedule(pixel_slices=0)
            plain = r.render_frame(cam)
            r.set_schedule(pixel_slices=slices)
            t0 = time.perf_counter()
            got = r.render_frame(cam)
            dt = time.perf_counter() - t0
            what = f"{cls.__name__} {w}x{h} tile {rank}/{world}, {slices} slices"
            assert dt < SLICE_FRAME_LIMIT_S, f"{what}: {dt:.1f} s"
            assert got.pixel_slices == (min(slices, _slice_units(spp)) if len(rows) else 1), what
            assert got.rays == plain.rays, what
            np.testing.assert_array_equal(got.rgba_f32, plain.rgba_f32, err_msg=what)
            np.testing.assert_array_equal(got.rgba_u8, plain.rgba_u8, err_msg=what)
            parts_f.append(got.rgba_f32), parts_b.append(got.rgba_u8)
            total += got.rays
        _assert_frames_equal(assemble_tiles(parts_f, h, world, strip), assemble_tiles(parts_b, h, world, strip), total, f, b, rays,
                             f"{cls.__name__} {w}x{h} over {world} tiles, {slices} slices")
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cls,kind", KINDS)
def test_a_lost_slice_hand_over_becomes_an_error_code_not_a_hung_gpu(dev_scenes, oracle, monkeypatch, cls, kind):
    """Every wait of a sliced kernel is for a slot a running or finished wave holds, so no wave can wait for ever — by design. The kernels bound
    the wait all the same: a wave that holds nothing but waiting lanes counts its looks and, after `wait_cap` of them (the product: > 15 s),
    lets its lanes run on with whatever the state buffer holds and leaves an error word: the frame call returns RT_ERR_HIP. Injected here
    (developer build): the cursor hands out second slices, but the cut mask is empty, so no lane ever ends a first slice and no state is ever
    written; the cap is lowered to a few thousand looks. The renderer renders the right frame again afterwards."""
    gs = dev_scenes("cornell")
    sd = gs.desc
    w, h, depth, spp = 96, 64, 6, 6
    cam = Camera.for_scene(sd, (w, h))
    f, b, rays = _oracle_frame(oracle, sd, w, h, kind, depth, spp)
    r = cls(gs, (w, h), depth, spp)
    r.set_schedule(pixel_slices=2)
    monkeypatch.setenv("RT_INJECT_SLICE_LOSS", "1")
    monkeypatch.setenv("RT_SLICE_WAIT_CAP", "3000")
    t0 = time.perf_counter()
    with pytest.raises(abi.RtError) as e:
        r.render_frame(cam)
    assert e.value.status == abi.RT_ERR_HIP and "slice" in str(e.value), e.value
    assert time.perf_counter() - t0 < 30.0
    monkeypatch.delenv("RT_INJECT_SLICE_LOSS")
    monkeypatch.delenv("RT_SLICE_WAIT_CAP")
    got = r.render_frame(cam)
    assert got.pixel_slices == 2
    _assert_frames_equal(got.rgba_f32, got.rgba_u8, got.rays, f, b, rays, f"{cls.__name__} after a lost hand-over")
    r.close()


@pytest.mark.gpu
def test_pixel_slices_are_chosen_by_tile_size_and_keep_the_frame(gpu_scenes, oracle, scene_cache):
    """Automatic slicing: none for a tile of at most ~1.25 pixels per resident lane (one generation of pixel chains: nothing is handed out
    later), several for a frame of several generations — and the frame, the tile split and the STATS instantiation are the same bits."""
    sd = scene_cache("atrium", detail=1)
    gs = gpu_scenes("atrium", detail=1)
    w, h, spp, depth = 1600, 904, 4, 10  # 1.45 M pixels on 393,216 lanes: 3.7 generations
    cam = Camera.for_scene(sd, (w, h))
    wf = WavefrontRenderer(gs, (w, h), depth, spp)  # the wavefront renderer's default schedule: sliced too, and the frame of its unsliced self
    wa = wf.render_frame(cam)
    assert wa.pixel_slices > 1 and wa.kernels["wf_finish"] == 1 and wa.kernels["wf_tile_order"] == 0
    wf.set_schedule(pixel_slices=0)
    wp = wf.render_frame(cam)
    assert wp.pixel_slices == 1 and wp.rays == wa.rays
    np.testing.assert_array_equal(wa.rgba_f32, wp.rgba_f32)
    wf.close()
    _assert_strips_equal_the_oracle(oracle, sd, abi.RT_RENDERER_WAVEFRONT, w, h, depth, spp, [("wavefront, automatic slices", wa.rgba_f32, wa.rgba_u8)], (3, 77),
                                    what="atrium 1600x904 sliced, wavefront")
    r = MegakernelRenderer(gs, (w, h), depth, spp)
    auto = r.render_frame(cam)
    assert auto.pixel_slices > 1
    r.set_schedule(pixel_slices=0)
    plain = r.render_frame(cam)
    assert plain.pixel_slices == 1 and plain.rays == auto.rays
    np.testing.assert_array_equal(auto.rgba_f32, plain.rgba_f32)
    np.testing.assert_array_equal(auto.rgba_u8, plain.rgba_u8)
    r.set_schedule(pixel_slices=-1)
    r.set_tile(0, 8, 8)  # 0.46 generations: the chain regime
    assert r.render_frame(cam).pixel_slices == 1
    r.set_tile(1, 2, 8)
    half = r.render_frame(cam)
    assert half.pixel_slices > 1
    np.testing.assert_array_equal(half.rgba_f32, plain.rgba_f32[r.global_rows()])
    r.close()
    # strips of the sliced frame against the oracle
    _assert_strips_equal_the_oracle(oracle, sd, abi.RT_RENDERER_MEGAKERNEL, w, h, depth, spp, [("automatic slices", auto.rgba_f32, auto.rgba_u8)], (0, 56, 112),
                                    what="atrium 1600x904 sliced")


@pytest.mark.gpu
def test_pixel_slices_in_the_instrumented_kernel_and_with_roulette(gpu_scenes, oracle, scene_cache, monkeypatch):
    sd = scene_cache("cornell")
    gs = gpu_scenes("cornell")
    w, h, spp, depth = 96, 64, 6, 8
    cam = Camera.for_scene(sd, (w, h))
    f, b, rays = _oracle_frame(oracle, sd, w, h, abi.RT_RENDERER_MEGAKERNEL, depth, spp)
    monkeypatch.setenv("RT_KERNEL_STATS", "1")
    r = MegakernelRenderer(gs, (w, h), depth, spp)
    r.set_schedule(pixel_slices=4)
    got = r.render_frame(cam)
    assert got.pixel_slices == 4
    _assert_frames_equal(got.rgba_f32, got.rgba_u8, got.rays, f, b, rays, "STATS instantiation, 4 slices")
    r.close()
    monkeypatch.delenv("RT_KERNEL_STATS")
    osc = oracle.OracleScene(sd)
    ocam = oracle.camera(w, h, sd.camera.position, sd.camera.direction, sd.camera.focal_length)
    f, b, rays = osc.render(ocam, abi.RT_RENDERER_MEGAKERNEL, depth, spp, use_bvh=False, rr_start=2)
    r = MegakernelRenderer(gs, (w, h), depth, spp)
    r.set_russian_roulette(2)
    r.set_schedule(pixel_slices=3)
    got = r.render_frame(cam)
    _assert_frames_equal(got.rgba_f32, got.rgba_u8, got.rays, f, b, rays, "roulette, 3 slices")
    r.close()


# ---- shading past the LDS-staged tables and without the packed shading word ------------------------------------------------------
# shade_hit (csrc/rt_device.h) reads a hit's material and normal matrix from the head of both tables staged in LDS (the megakernel and
# k_wf_finish: kLdsMats = 24 materials, kLdsNm = 8 distinct matrices) only when every hit of the round is inside it; any other round reads them
# from memory, and a scene of more than 4096 materials (or 2^20 instances) has no packed shading word: the material then comes through the
# instance record. rtamd.scenes.table_scene puts frames on either side of those limits, and the developer library says which side
# (rt_dev_scene_tables; the product library builds the same tables from the same host code).
TABLE_W, TABLE_H, TABLE_SPP, TABLE_DEPTH = 96, 72, 3, 6
TABLE_CASES = [  # (id, table_scene arguments, (packed_mat, lds_nm, lds_mats) of the device scene)
    ("staged", dict(n_mats=24, n_rows=8), (1, 8, 24)),
    ("one_past", dict(n_mats=25, n_rows=9), (1, 8, 24)),
    ("many", dict(n_mats=300, n_rows=64, n_inst=300), (1, 8, 24)),
    ("packed_4096", dict(n_mats=4096, n_rows=12), (1, 8, 24)),
    ("unpacked_4097", dict(n_mats=4097, n_rows=12), (0, 0, 0)),
]
TABLE_SCHEDULES = [  # (what, renderer, schedule)
    ("megakernel", MegakernelRenderer, dict(pixel_slices=0)),
    ("megakernel, 3 slices", MegakernelRenderer, dict(pixel_slices=3)),
    ("wavefront, one launch", WavefrontRenderer, dict(pixel_slices=0, cost_order=0)),
    ("wavefront, one launch, 3 slices", WavefrontRenderer, dict(pixel_slices=3, cost_order=0)),
    ("per bounce", WavefrontRenderer, dict(finish_depth=ALL_BOUNCES)),
    ("per bounce, fused", WavefrontRenderer, dict(finish_depth=ALL_BOUNCES, fused_bounce=True)),
    ("per bounce, reorder + matsort", WavefrontRenderer, dict(finish_depth=ALL_BOUNCES, reorder=True, matsort=True)),
]


def _table_hits(oracle, sd, packed):
    """(material, table row or None) of the hit under every pixel centre of the TABLE_W x TABLE_H frame that hits, mapped on the host:
    triangle -> instance -> material, and the row through the scene's shading words."""
    cam = oracle.camera(TABLE_W, TABLE_H, sd.camera.position, sd.camera.direction, sd.camera.focal_length)
    x, y = np.meshgrid(np.arange(TABLE_W, dtype=np.float32), np.arange(TABLE_H, dtype=np.float32))
    p00, du, dv, c = (np.array(v, np.float32) for v in (cam.pixel00, cam.delta_u, cam.delta_v, cam.center))
    d = p00 + x.reshape(-1, 1) * du + y.reshape(-1, 1) * dv - c
    tri = oracle.OracleScene(sd).intersect(np.broadcast_to(c, d.shape), d, use_bvh=False)[3]
    tri = tri[tri != NO_TRI]
    return sd.inst_material[sd.tri_instance[tri]].astype(np.int64), (packed["words"][tri] & 0xFFFFF).astype(np.int64) if packed else None


def _assert_table_schedule_ran(got, cls, sched, what):
    k = got.kernels
    if "finish_depth" not in sched:  # one launch per frame
        assert got.pixel_slices == (3 if sched["pixel_slices"] == 3 else 1), what
        if cls is MegakernelRenderer:
            assert k["megakernel"] == 1, (what, k)
            return
        assert got.stream_lanes == 1 and k["wf_finish"] == 1 and k["wf_extend"] == k["wf_shade"] == k["wf_shoot"] == 0, (what, k)
    else:  # a launch (pair) per bounce all the way down
        lanes = got.stream_lanes
        pairs = lanes * TABLE_SPP * TABLE_DEPTH
        assert lanes == PER_BOUNCE_LANES and got.finish_depth == TABLE_DEPTH and k["wf_finish"] == 0, (what, k)
        fused = bool(sched.get("fused_bounce"))
        assert k["wf_extend"] == k["wf_shade"] == (0 if fused else pairs) and k["wf_shoot"] == (pairs if fused else 0), (what, k)
        assert k["wf_shade_reorder"] == (pairs if sched.get("reorder") else 0), (what, k)
        assert k["wf_shade_matsort"] == (pairs if sched.get("matsort") else 0), (what, k)
    assert sum(k.values()) - k["wf_shade_reorder"] - k["wf_shade_matsort"] - k["wf_finish_requeue"] == got.launches, (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("case,kw,tables", TABLE_CASES, ids=[c[0] for c in TABLE_CASES])
def test_shading_past_the_staged_tables_and_the_packed_word(gpu_scenes, dev_scenes, oracle, case, kw, tables):
    """Each table configuration on every schedule: the megakernel unsliced and sliced, the wavefront renderer's one launch unsliced and sliced
    (both stage the tables), its per-bounce schedules split and fused (the dense SHADE kernel: memory only), and re-ordered with the material
    sort, whose key reads the material with and without the packed word. Frame, unorm8 image and ray count bit for bit the oracle's (brute
    force), and the launch counts prove each schedule ran. The scene's table state and the hits of its primary rays prove which shading path
    the frame has to take."""
    t = dev_scenes("tables", **kw).shading_tables()
    assert (t["packed_mat"], t["lds_nm"], t["lds_mats"]) == tables
    gs = gpu_scenes("tables", **kw)
    sd = gs.desc
    mats, rows = _table_hits(oracle, sd, t if t["packed_mat"] else None)
    staged = (mats < 24) & (rows < 8) if rows is not None else np.zeros(mats.shape, bool)
    if case == "staged":
        assert staged.all() and t["rows"].shape[0] == 8
    elif case == "one_past":
        assert (mats == 24).any() and (rows == 8).any() and staged.any()
    elif case == "many":
        assert (mats >= 24).any() and (rows >= 8).any() and (~staged).mean() > 0.5
    elif case == "packed_4096":
        assert (mats == 4095).any() and (mats < 24).any() and staged.any()
    else:
        assert (mats == 4096).any() and (mats < 24).any()
    cam = Camera.for_scene(sd, (TABLE_W, TABLE_H))
    want = {kind: _oracle_frame(oracle, sd, TABLE_W, TABLE_H, kind, TABLE_DEPTH, TABLE_SPP, use_bvh=False) for _cls, kind in KINDS}
    for what, cls, sched in TABLE_SCHEDULES:
        what = f"{case}: {what}"
        r = cls(gs, (TABLE_W, TABLE_H), TABLE_DEPTH, TABLE_SPP)
        r.set_schedule(**sched)
        got = r.render_frame(cam)
        _assert_table_schedule_ran(got, cls, sched, what)
        f, b, rays = want[cls.KIND]
        _assert_frames_equal(got.rgba_f32, got.rgba_u8, got.rays, f, b, rays, what)
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case,kw,tables", [c for c in TABLE_CASES if c[1]["n_mats"] > 24], ids=[c[0] for c in TABLE_CASES if c[1]["n_mats"] > 24])
def test_scatter_probe_reads_high_material_indices(gpu_scenes, oracle, case, kw, tables):
    """rt_probe_scatter on materials 24, 4095 and 4096 where the scene has them (and its first and last): the probe and the oracle read the
    same record at high indices, bit for bit."""
    gs = gpu_scenes("tables", **kw)
    sd = gs.desc
    osc = oracle.OracleScene(sd)
    rng = np.random.default_rng(24)
    n = 4096
    dirs, nrm = _unit(rng.normal(size=(n, 3))), _unit(rng.normal(size=(n, 3)))
    uv = rng.uniform(-3, 3, (n, 2)).astype(np.float32)
    seeds = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    for m in sorted({0, 24, 4095, 4096, len(sd.materials) - 1} & set(range(len(sd.materials)))):
        g, e = gs.scatter(m, dirs, nrm, uv, seeds), osc.scatter(m, dirs, nrm, uv, seeds)
        for a, b, part in zip(g, e, ("ok flag", "direction", "attenuation", "rng state")):
            np.testing.assert_array_equal(a, b, err_msg=f"{case} material {m}: {part}")
