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


def scene_bounds(sd):
    """(lo, hi, scale) of the world triangles: the bounds and max(largest extent, largest |coordinate|), the scene scale of the contract range"""
    v = sd.world_triangles().reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    return lo, hi, float(max((hi - lo).max(), np.abs(lo).max(), np.abs(hi).max()))


def _directed_cases():
    """Directions a camera fan never holds, unnormalised fp32: the six axes and the twelve two-axis diagonals with exact +0 and -0 in the
    other components, components that are half subnormals, and components on half rounding ties (1 + 2^-11 lies between 1 and 1 + 2^-10
    and goes to the even 1, 1 + 3 * 2^-11 between 1 + 2^-10 and 1 + 2^-9 and goes to the even 1 + 2^-9: truncation gives 1 and 1 + 2^-10,
    round-half-up 1 + 2^-10 and 1 + 2^-9; 2^-25 and 3 * 2^-25 are the same pair among the subnormals)."""
    d = []
    for a in range(3):
        for sgn in (1.0, -1.0):
            for zero in (0.0, -0.0):
                v = [zero] * 3
                v[a] = sgn
                d.append(v)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        for sa in (1.0, -1.0):
            for sb in (1.0, -1.0):
                v = [0.0 if sa > 0 else -0.0] * 3
                v[a], v[b] = sa, sb
                d.append(v)
    d += [[3e-6, 1.0, 0.5], [-1.0, -3e-6, 2e-7], [0.25, 3e-6, -3e-6], [3e-6, 3e-6, -5e-6], [6.0e-5, -1.0, 6.1e-5]]
    t1, t3 = 1.0 + 2.0 ** -11, 1.0 + 3.0 * 2.0 ** -11
    d += [[t1, t3, -t1], [-t3, t1, t3], [t1 * 0.125, -t3 * 0.125, 0.125], [t3 * 32.0, t1 * 32.0, -32.0], [t1, 0.0, t3], [-t1, -t3, -0.0],
          [2.0 ** -25, 1.0, -3.0 * 2.0 ** -25], [3.0 * 2.0 ** -25, -2.0 ** -25, -1.0]]
    return np.array(d, f32)


def probe_mix(sd, n, seed):
    """The rays of light probes and bakers rather than of a camera: (org (n, 3) float32, dirs (n, 3) float32, rng (n,) uint32), shuffled, so
    that every prefix is a mix too. Directions are NOT rounded to half: that is the kernel's job and the oracle's (R3).
      n // 2  origins uniform inside the scene's bounds, directions uniform on the sphere times a length log-uniform in [1e-2, 1e2]
      n // 4  origins on triangle surfaces (random world triangles, random barycentrics), directions alternately into the front and the
              back hemisphere of the face, same lengths: half of them start inside whatever closed mesh the face belongs to
      n // 8  origins outside the bounds, up to 90 scene scales out on one, two or three axes (inside the 100 of the contract range), half
              aimed at the bounds' centre and half away from it
      rest    _directed_cases(), repeated, from origins inside the bounds
    States: random non-zero words; entries 0 to 3 hold 0, 1, 0x80000000 and 0xFFFFFFFF."""
    g = np.random.default_rng(seed)
    lo, hi, scale = scene_bounds(sd)
    centre = 0.5 * (lo + hi)

    def sphere(k):
        v = g.normal(size=(k, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    def lengths(k):
        return 10.0 ** g.uniform(-2.0, 2.0, size=(k, 1))

    n_in, n_surf, n_out = n // 2, n // 4, n // 8
    n_dir = n - n_in - n_surf - n_out
    org, dirs = [], []
    org.append(g.uniform(lo, hi, size=(n_in, 3)))
    dirs.append(sphere(n_in) * lengths(n_in))
    tris = sd.world_triangles()[g.integers(0, sd.n_triangles, n_surf)]
    u, v = g.uniform(size=n_surf), g.uniform(size=n_surf)
    fold = u + v > 1.0
    u, v = np.where(fold, 1.0 - u, u)[:, None], np.where(fold, 1.0 - v, v)[:, None]
    e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    org.append(tris[:, 0] + u * e1 + v * e2)
    d = sphere(n_surf)
    side = np.where(np.arange(n_surf) % 2 == 0, 1.0, -1.0)  # the hemisphere the direction has to point into
    flip = np.sign(np.einsum("ij,ij->i", d, np.cross(e1, e2))) * side < 0
    dirs.append(np.where(flip[:, None], -d, d) * lengths(n_surf))
    o = g.uniform(lo, hi, size=(n_out, 3))
    axes = g.integers(1, 8, n_out)  # which axes leave the bounds: at least one
    out = g.uniform(0.0, 90.0, size=(n_out, 3)) * scale
    below = g.integers(0, 2, size=(n_out, 3)) == 1
    far = np.where(below, lo - out, hi + out)
    o = np.where((axes[:, None] >> np.arange(3)) & 1 == 1, far, o)
    org.append(o)
    to = centre - o
    to /= np.linalg.norm(to, axis=1, keepdims=True)
    dirs.append(np.where((np.arange(n_out) % 2 == 0)[:, None], to, -to) * lengths(n_out))
    cases = _directed_cases()
    org.append(g.uniform(lo, hi, size=(n_dir, 3)))
    dirs.append(cases[np.arange(n_dir) % len(cases)])
    perm = g.permutation(n)
    org = np.concatenate(org).astype(f32)[perm]
    dirs = np.concatenate([np.asarray(x, f32) for x in dirs])[perm]
    state = g.integers(1, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    state[:4] = np.array([0, 1, 0x80000000, 0xFFFFFFFF], np.uint32)[:min(n, 4)]
    return np.ascontiguousarray(org), np.ascontiguousarray(dirs), state


PROBE_N, PROBE_SEED = 4096 + 33, 17  # 65 chunks of 64 rays: one partial; 129 or 130 rays per shard
_PROBES = {}


def probe_case(name):
    """(description, the oracle's scene, probe_mix(PROBE_N, PROBE_SEED)) of "cornell", "atrium" (coarse) or "tables", built once per process"""
    if name not in _PROBES:
        from oracle import oracle as O
        sd = scenes.table_scene() if name == "tables" else scenes.get_scene(name, **({"coarse": True} if name == "atrium" else {}))
        _PROBES[name] = (sd, O.OracleScene(sd), probe_mix(sd, PROBE_N, PROBE_SEED))
    return _PROBES[name]


_EXPECTED = {}


def probe_expected(name, max_depth, samples, rr_start):
    """The oracle's path query on the scene's probe mix, computed once per process and shared (read only) by the tests that compare with it"""
    key = (name, max_depth, samples, rr_start)
    if key not in _EXPECTED:
        _, osc, (org, dirs, state) = probe_case(name)
        out = osc.trace_paths(org, dirs, state, max_depth, samples=samples, rr_start=rr_start)
        for a in out.values():
            a.setflags(write=False)
        _EXPECTED[key] = out
    return _EXPECTED[key]


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
