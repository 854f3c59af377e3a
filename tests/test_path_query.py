"""Path queries (include/rt_mi355x.h: rt_trace_paths[_device]) without a GPU: the exported entry points, the refusals in front of the device,
the Python wrappers' shape checks, the numpy model of the camera ray that tests/test_gpu_path_query.py chains queries with, and the listing
of the kernel's unit (ISA hazard scan, resources as DESIGN.md §17 states them)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from rtamd import abi, scenes
from rtamd.renderer import Scene

REPO = Path(__file__).resolve().parent.parent
f32 = np.float32
K_PATH_QUERY = "_ZN2rt12k_path_queryENS_8SceneDevENS_7PathDevE"


# ---- the model the GPU tests share ------------------------------------------------------------------------------------------------------
def xorshift_model(state):
    """XorShift32State::operator() (oracle_rt.cpp: Rng::next) on an array of states: (the floats drawn, the states after)"""
    x = np.array(state, np.uint32, copy=True)
    x ^= x << np.uint32(13)
    x ^= x >> np.uint32(17)
    x ^= x << np.uint32(5)
    return x.astype(f32) * f32(1.0 / 4294967296.0), x


def get_ray_model(cam, x, y, state):
    """get_ray (oracle_rt.cpp:422-439) for arrays of pixels: camera_ray's pixel centre, two xorshift draws and the direction BEFORE the half
    rounding (the path query rounds it). cam: an rt_camera. Every operation is one fp32 operation, in the oracle's order.
    -> (dir (n, 3) float32, state')"""
    p00, du, dv, ce = (np.array(list(v), f32) for v in (cam.pixel00, cam.delta_u, cam.delta_v, cam.center))
    xf, yf = np.asarray(x).astype(f32)[:, None], np.asarray(y).astype(f32)[:, None]
    pixel_center = (p00[None, :] + xf * du[None, :]) + yf * dv[None, :]
    u0, state = xorshift_model(state)
    u1, state = xorshift_model(state)
    px, py = (f32(-0.5) + u0)[:, None], (f32(-0.5) + u1)[:, None]
    sq = px * du[None, :] + py * dv[None, :]
    pixel_sample = pixel_center + sq
    d = pixel_sample - ce[None, :]
    assert d.dtype == f32
    return d, state


def pixel_seed_model(x, y, w, h, megakernel, salt=0):
    """pixel_seed (rt_device.h) + rt_renderer_set_frame_seed's salt x 0x9E3779B9, modulo 2^32"""
    x, y = np.asarray(x).astype(np.uint64), np.asarray(y).astype(np.uint64)
    base = x * np.uint64((h + 7) // 8 * 8) + y if megakernel else x + y * np.uint64(w)
    return ((base + np.uint64(salt) * np.uint64(0x9E3779B9)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


# ---- the surface --------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_prototyped(rtlib, devlib):
    header = (REPO / "include" / "rt_mi355x.h").read_text()
    assert "typedef struct rt_path_query {" in header
    for name in ("rt_trace_paths", "rt_trace_paths_device"):
        assert re.search(rf"^int {name}\(rt_scene\* scene, const rt_path_query\* q", header, re.M), name
        assert name in abi.PROTOTYPES
        for lib in (rtlib, devlib):
            assert hasattr(lib, name), name
    assert C.sizeof(abi.rt_path_query) == 64
    assert [f[0] for f in abi.rt_path_query._fields_] == ["n", "max_depth", "samples", "rr_start", "org", "dir", "rng", "rng_out", "radiance", "rays"]
    assert rtlib.rt_abi_version() == 8 and "#define RT_ABI_VERSION 8" in header


def _query(n=4, max_depth=5, samples=1, rr_start=0, org=True, dirs=True, rng=True, rng_out=True, radiance=True, rays=True, keep=None):
    bufs = {"org": np.zeros((4, 3), f32), "dir": np.ones((4, 3), f32), "rng": np.arange(1, 5, dtype=np.uint32),
            "rng_out": np.zeros(4, np.uint32), "radiance": np.zeros((4, 3), f32), "rays": np.zeros(4, np.uint32)}
    if keep is not None:
        keep.append(bufs)
    q = abi.rt_path_query(n=n, max_depth=max_depth, samples=samples, rr_start=rr_start)
    for name, want in (("org", org), ("dir", dirs), ("rng", rng), ("rng_out", rng_out), ("radiance", radiance), ("rays", rays)):
        setattr(q, name, bufs[name].ctypes.data if want else None)
    return q


def _err(lib):
    return lib.rt_last_error().decode()


@pytest.mark.parametrize("entry", ["rt_trace_paths", "rt_trace_paths_device"])
def test_refusals_come_before_any_device_call(rtlib, entry):
    """On a host-only scene no device call can succeed, so every status below was decided in front of the device: RT_ERR_INVALID with the
    cause named for a NULL scene, query or required pointer and for max_depth == 0 or samples == 0; RT_ERR_NO_DEVICE for a well-formed
    query (the arguments are checked first); RT_OK for n == 0."""
    s = Scene(scenes.get_scene("cornell"), device=-1)
    fn = getattr(rtlib, entry)
    call = (lambda h, q: fn(h, q)) if entry == "rt_trace_paths" else (lambda h, q: fn(h, q, None))
    keep = []
    inv = abi.RT_ERR_INVALID
    assert call(None, C.byref(_query(keep=keep))) == inv and "null argument" in _err(rtlib)
    assert call(s.h, None) == inv and "null argument" in _err(rtlib)
    assert call(None, None) == inv
    for kw, word in (({"org": False}, "org"), ({"dirs": False}, "dir"), ({"rng": False}, "rng"), ({"radiance": False}, "radiance"),
                     ({"max_depth": 0}, "max_depth"), ({"samples": 0}, "samples")):
        assert call(s.h, C.byref(_query(keep=keep, **kw))) == inv, kw
        assert word in _err(rtlib), (kw, _err(rtlib))
    for kw in ({}, {"rng_out": False}, {"rays": False}, {"rng_out": False, "rays": False}, {"samples": 7, "rr_start": 3}, {"max_depth": 1}):
        assert call(s.h, C.byref(_query(keep=keep, **kw))) == abi.RT_ERR_NO_DEVICE, kw
        assert "host-only" in _err(rtlib)
    assert call(s.h, C.byref(_query(n=0, keep=keep))) == abi.RT_OK
    assert call(s.h, C.byref(_query(n=0, org=False, dirs=False, rng=False, radiance=False, keep=keep))) == abi.RT_OK
    s.close()


def test_python_wrappers_refuse_wrong_shapes(rtlib):
    s = Scene(scenes.get_scene("cube"), device=-1)
    org, dirs, rng = np.zeros((2, 3), f32), np.ones((2, 3), f32), np.ones(2, np.uint32)
    with pytest.raises(abi.RtError) as e:
        s.trace_paths(org, dirs, rng, 5)
    assert e.value.status == abi.RT_ERR_NO_DEVICE
    for bad in ((org, np.ones((3, 3), f32), rng), (org, dirs, np.ones(3, np.uint32)), (org, dirs, np.ones((2, 1), np.uint32)),
                (np.zeros(6, f32), np.ones(6, f32), rng), (np.zeros((2, 4), f32), np.ones((2, 4), f32), rng), (org, dirs, np.ones(2, f32))):
        with pytest.raises(ValueError):
            s.trace_paths(*bad, 5)
    for kw in ({"max_depth": 0}, {"max_depth": 5, "samples": 0}):
        with pytest.raises(abi.RtError) as e:
            s.trace_paths(org, dirs, rng, **kw)
        assert e.value.status == abi.RT_ERR_INVALID
    out = s.trace_paths(np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros(0, np.uint32), 5)
    assert out["radiance"].shape == (0, 3) and out["rng"].shape == (0,) and out["rays"].shape == (0,)
    assert out["radiance"].dtype == f32 and out["rng"].dtype == np.uint32 and out["rays"].dtype == np.uint32
    with pytest.raises(abi.RtError) as e:
        s.trace_paths_device(5, 0, 0, 0, 0, 5)
    assert e.value.status == abi.RT_ERR_INVALID
    s.close()


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
def test_xorshift_model_equals_the_oracle(oracle):
    rng = np.random.default_rng(3)
    seeds = np.concatenate([np.array([1, 2, 0x80000000, 0xFFFFFFFF, 0x9E3779B9], np.uint32), rng.integers(1, 2**32, 3000, dtype=np.uint64).astype(np.uint32)])
    u, st = xorshift_model(seeds)
    u2, st2 = xorshift_model(st)
    for k, seed in enumerate(seeds):
        vals, end = oracle.xorshift(int(seed), 2)
        assert vals[0] == u[k] and vals[1] == u2[k] and end == int(st2[k]), hex(int(seed))
    assert u.dtype == f32 and st.dtype == np.uint32


def test_get_ray_model_draws_twice_and_starts_at_the_pixel_centre(oracle):
    sd = scenes.get_scene("cornell")
    w, h = 48, 32
    cam = oracle.camera(w, h, sd.camera.position, sd.camera.direction, sd.camera.focal_length)
    ys, xs = np.mgrid[0:h, 0:w]
    x, y = xs.ravel(), ys.ravel()
    seeds = pixel_seed_model(x, y, w, h, megakernel=True) + np.uint32(1)
    d, st = get_ray_model(cam, x, y, seeds)
    assert d.shape == (w * h, 3) and d.dtype == f32
    for k in (0, 47, 48, w * h - 1):  # the state has moved by exactly two draws
        assert oracle.xorshift(int(seeds[k]), 2)[1] == int(st[k])
    # the sample lies within half a pixel of the pixel's centre on both image axes
    p00, du, dv, ce = (np.array(list(v), np.float64) for v in (cam.pixel00, cam.delta_u, cam.delta_v, cam.center))
    centre = p00 + x[:, None] * du + y[:, None] * dv - ce
    off = d.astype(np.float64) - centre
    assert (np.abs(off @ du / (du @ du)) <= 0.5 + 1e-4).all() and (np.abs(off @ dv / (dv @ dv)) <= 0.5 + 1e-4).all()
    assert np.abs(off @ du / (du @ du)).max() > 0.45
    # seeds: the megakernel's column-major seed with the height rounded up to 8, the wavefront's row-major one, the salt's golden-ratio step
    assert int(pixel_seed_model([3], [5], 64, 36, True)[0]) == 3 * 40 + 5
    assert int(pixel_seed_model([3], [5], 64, 36, False)[0]) == 3 + 5 * 64
    assert int(pixel_seed_model([3], [5], 64, 36, False, salt=5)[0]) == (3 + 5 * 64 + 5 * 0x9E3779B9) % 2**32


# ---- the listing --------------------------------------------------------------------------------------------------------------------------
def test_path_query_kernel_passes_the_isa_hazard_scan_with_the_resources_design_states(tmp_path):
    """k_path_query (rt_path_query.hip) through tests/test_isa_hazards.py's checker: it carries the asm node fetch and breaks none of its
    rules. Its registers, scratch and LDS are the figures of DESIGN.md §17, read from the listing's metadata and from DESIGN.md itself."""
    from test_denoise import _listing
    from test_isa_hazards import _check
    from test_svgf import _metadata
    lines = _listing("rt_path_query.hip", tmp_path)
    groups = _check(lines)
    assert list(groups) == [K_PATH_QUERY] and groups[K_PATH_QUERY] >= 1, groups
    meta = "\n".join(lines)
    got = {k: _metadata(meta, K_PATH_QUERY, k) for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    design = (REPO / "DESIGN.md").read_text()
    m = re.search(r"`k_path_query`: (\d+) VGPRs, (\d+) spilled, (\d+) bytes of scratch per lane, ([\d,]+) bytes of LDS per workgroup", design)
    assert m, "DESIGN.md states k_path_query's resources in one sentence"
    stated = {"vgpr_count": int(m.group(1)), "vgpr_spill_count": int(m.group(2)), "private_segment_fixed_size": int(m.group(3)),
              "group_segment_fixed_size": int(m.group(4).replace(",", ""))}
    assert got == stated
    assert got["vgpr_count"] <= 80  # 6 waves per SIMD (512 registers / 6, in blocks of 8)
    assert 3 * got["group_segment_fixed_size"] <= 160 * 1024  # three 512-thread workgroups per CU: 24 waves = 6 per SIMD
