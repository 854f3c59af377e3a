"""Gather queries (include/rt_mi355x.h: rt_gather_paths[_device]) without a GPU: the exported entry points and the struct layout, the
refusals in front of the device, the Python wrappers' shape checks, the numpy model tests/test_gpu_gather.py compares the device with (the
diffuse bounce's unit vector, checked against the oracle's scatter, around the oracle's path query), what the point mix reaches, the listing
of the kernel's unit (ISA hazard scan, resources as DESIGN.md §18 states them) and the baker's points."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rtamd import abi, bake, scenes
from rtamd.renderer import Scene
from test_path_query import _directed_cases, probe_case, scene_bounds, xorshift_model

REPO = Path(__file__).resolve().parent.parent
f32 = np.float32
K_PATH_GATHER = "_ZN2rt13k_path_gatherENS_8SceneDevENS_9GatherDevE"
K_PATH_QUERY = "_ZN2rt12k_path_queryENS_8SceneDevENS_7PathDevE"


# ---- the model both files share ---------------------------------------------------------------------------------------------------------
def unit_vector_model(state):
    """random_unit_vector (oracle_rt.cpp: Rng::unit_vector; rt_device.h: rng_unit_vector) on an array of states: three draws x, y, z of
    -1 + 2 * u each, then v * (1 / sqrt((x*x + y*y) + z*z)), every operation one fp32 operation. -> (unit (n, 3) float32, the states after)"""
    comp = []
    for _ in range(3):
        u, state = xorshift_model(state)
        comp.append(f32(-1.0) + f32(2.0) * u)
    x, y, z = comp
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = f32(1.0) / np.sqrt((x * x + y * y) + z * z)
        v = np.stack([x * inv, y * inv, z * inv], 1)
    assert v.dtype == f32
    return v, state


def gather_model(trace, pos, nrm, state, depth, samples, rr):
    """The gather query as a chain of path queries (include/rt_mi355x.h): per sample draw the unit vector from the running states, trace one
    path from (pos, nrm + unit) with them, add. `trace` is OracleScene.trace_paths or Scene.trace_paths. -> {"radiance", "rng", "rays"}"""
    pos, nrm = np.ascontiguousarray(pos, f32), np.ascontiguousarray(nrm, f32)
    state = np.array(state, np.uint32, copy=True)
    total = np.zeros_like(pos)
    rays = np.zeros(len(pos), np.uint32)
    for _ in range(samples):
        u, state = unit_vector_model(state)
        out = trace(pos, nrm + u, state, depth, samples=1, rr_start=rr)
        total = total + out["radiance"]
        rays = rays + out["rays"]
        state = out["rng"]
    return {"radiance": total / f32(samples), "rng": state, "rays": rays}


SPECIAL_NORMALS = np.array([[0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [1e5, 0.0, 0.0], [0.0, -7e4, 1.0], [1e-8, 1e-8, -1e-8]], f32)


def point_mix(sd, n, seed):
    """What a baker sends, shuffled, so that every prefix is a mix too: (pos (n, 3) float32, normal (n, 3) float32, rng (n,) uint32).
      n // 2  points on random world triangles at random barycentrics, unit face normals alternately front and back: the back ones start
              inside closed meshes or behind walls
      n // 4  points uniform inside the bounds, normals uniform on the sphere times a length log-uniform in [1e-2, 1e2]
      n // 8  points up to 90 scene scales outside the bounds on one to three axes, the normal towards the centre or away from it
      rest    points inside the bounds with test_path_query's _directed_cases() as normals and SPECIAL_NORMALS: zero normals of both signs
              (the lobe is the unit vector alone), 1e5 and -7e4 (the direction overflows half: the sky after one ray), 1e-8 (lost in the add)
    States: random non-zero words; entries 0 to 3 hold 0, 1, 0x80000000 and 0xFFFFFFFF."""
    g = np.random.default_rng(seed)
    lo, hi, scale = scene_bounds(sd)
    centre = 0.5 * (lo + hi)

    def sphere(k):
        v = g.normal(size=(k, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    n_surf, n_in, n_out = n // 2, n // 4, n // 8
    n_dir = n - n_surf - n_in - n_out
    pos, nrm = [], []
    tris = sd.world_triangles()[g.integers(0, sd.n_triangles, n_surf)]
    u, v = g.uniform(size=n_surf), g.uniform(size=n_surf)
    fold = u + v > 1.0
    u, v = np.where(fold, 1.0 - u, u)[:, None], np.where(fold, 1.0 - v, v)[:, None]
    e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    pos.append(tris[:, 0] + u * e1 + v * e2)
    face = np.cross(e1, e2)
    face /= np.linalg.norm(face, axis=1, keepdims=True)
    nrm.append(face * np.where(np.arange(n_surf) % 2 == 0, 1.0, -1.0)[:, None])
    pos.append(g.uniform(lo, hi, size=(n_in, 3)))
    nrm.append(sphere(n_in) * 10.0 ** g.uniform(-2.0, 2.0, size=(n_in, 1)))
    o = g.uniform(lo, hi, size=(n_out, 3))
    axes = g.integers(1, 8, n_out)  # which axes leave the bounds: at least one
    out = g.uniform(0.0, 90.0, size=(n_out, 3)) * scale
    below = g.integers(0, 2, size=(n_out, 3)) == 1
    o = np.where((axes[:, None] >> np.arange(3)) & 1 == 1, np.where(below, lo - out, hi + out), o)
    pos.append(o)
    to = centre - o
    to /= np.linalg.norm(to, axis=1, keepdims=True)
    nrm.append(np.where((np.arange(n_out) % 2 == 0)[:, None], to, -to))
    cases = np.concatenate([_directed_cases(), SPECIAL_NORMALS])
    pos.append(g.uniform(lo, hi, size=(n_dir, 3)))
    nrm.append(cases[np.arange(n_dir) % len(cases)])
    perm = g.permutation(n)
    pos = np.concatenate(pos).astype(f32)[perm]
    nrm = np.concatenate([np.asarray(x, f32) for x in nrm])[perm]
    state = g.integers(1, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    state[:4] = np.array([0, 1, 0x80000000, 0xFFFFFFFF], np.uint32)[:min(n, 4)]
    return np.ascontiguousarray(pos), np.ascontiguousarray(nrm), state


MIX_N, MIX_SEED = 4096 + 33, 29  # 65 chunks of 64 entries: one partial; 129 or 130 entries per shard
DEPTH = 5
_MIX, _EXPECTED = {}, {}


def mix_case(name):
    """(description, the oracle's scene, point_mix(MIX_N, MIX_SEED)) of "cornell", "atrium" (coarse) or "tables", built once per process"""
    if name not in _MIX:
        sd, osc, _ = probe_case(name)
        _MIX[name] = (sd, osc, point_mix(sd, MIX_N, MIX_SEED))
    return _MIX[name]


def mix_expected(name, max_depth, samples, rr_start):
    """gather_model over the oracle's path query on the scene's point mix, computed once per process and shared read-only"""
    key = (name, max_depth, samples, rr_start)
    if key not in _EXPECTED:
        _, osc, (pos, nrm, state) = mix_case(name)
        out = gather_model(osc.trace_paths, pos, nrm, state, max_depth, samples, rr_start)
        for a in out.values():
            a.setflags(write=False)
        _EXPECTED[key] = out
    return _EXPECTED[key]


def steps(state, k):
    for _ in range(k):
        _, state = xorshift_model(state)
    return state


def sky_mean(sky, samples):
    """the sky summed `samples` times from +0 and divided, as the kernel's colour sum does"""
    total = np.zeros(3, f32)
    for _ in range(samples):
        total = total + np.asarray(sky, f32)
    return total / f32(samples)


# ---- the surface --------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_prototyped(rtlib, devlib, tmp_path):
    header = (REPO / "include" / "rt_mi355x.h").read_text()
    assert "typedef struct rt_gather_query {" in header
    for name in ("rt_gather_paths", "rt_gather_paths_device"):
        assert re.search(rf"^int {name}\(rt_scene\* scene, const rt_gather_query\* q", header, re.M), name
        assert name in abi.PROTOTYPES
        for lib in (rtlib, devlib):
            assert hasattr(lib, name), name
    fields = ["n", "max_depth", "samples", "rr_start", "pos", "normal", "rng", "rng_out", "radiance", "rays"]
    assert [f[0] for f in abi.rt_gather_query._fields_] == fields
    assert rtlib.rt_abi_version() == 8 and "#define RT_ABI_VERSION 8" in header
    # the layout, measured by compiling a C program against the header
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_mi355x.h"\nint main(void){printf("%zu\\n", sizeof(rt_gather_query));' +
                   "".join(f'printf("%zu\\n", offsetof(rt_gather_query, {f}));' for f in fields) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", str(REPO / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(abi.rt_gather_query)] + [getattr(abi.rt_gather_query, f).offset for f in fields]
    assert got[0] == 64


def _query(n=4, max_depth=5, samples=1, rr_start=0, pos=True, normal=True, rng=True, rng_out=True, radiance=True, rays=True, keep=None):
    bufs = {"pos": np.zeros((4, 3), f32), "normal": np.ones((4, 3), f32), "rng": np.arange(1, 5, dtype=np.uint32),
            "rng_out": np.zeros(4, np.uint32), "radiance": np.zeros((4, 3), f32), "rays": np.zeros(4, np.uint32)}
    if keep is not None:
        keep.append(bufs)
    q = abi.rt_gather_query(n=n, max_depth=max_depth, samples=samples, rr_start=rr_start)
    for name, want in (("pos", pos), ("normal", normal), ("rng", rng), ("rng_out", rng_out), ("radiance", radiance), ("rays", rays)):
        setattr(q, name, bufs[name].ctypes.data if want else None)
    return q


def _err(lib):
    return lib.rt_last_error().decode()


@pytest.mark.parametrize("entry", ["rt_gather_paths", "rt_gather_paths_device"])
def test_refusals_come_before_any_device_call(rtlib, entry):
    """On a host-only scene no device call can succeed, so every status below was decided in front of the device, in the header's order:
    RT_ERR_INVALID with the cause named for a NULL scene, query or required pointer and for max_depth == 0 or samples == 0;
    RT_ERR_NO_DEVICE for a well-formed query (the arguments are checked first); RT_OK for n == 0."""
    s = Scene(scenes.get_scene("cornell"), device=-1)
    fn = getattr(rtlib, entry)
    call = (lambda h, q: fn(h, q)) if entry == "rt_gather_paths" else (lambda h, q: fn(h, q, None))
    keep = []
    inv = abi.RT_ERR_INVALID
    assert call(None, C.byref(_query(keep=keep))) == inv and "null argument" in _err(rtlib)
    assert call(s.h, None) == inv and "null argument" in _err(rtlib)
    assert call(None, None) == inv
    for kw, word in (({"pos": False}, "pos"), ({"normal": False}, "normal"), ({"rng": False}, "rng"), ({"radiance": False}, "radiance"),
                     ({"max_depth": 0}, "max_depth"), ({"samples": 0}, "samples")):
        assert call(s.h, C.byref(_query(keep=keep, **kw))) == inv, kw
        assert word in _err(rtlib), (kw, _err(rtlib))
    assert call(s.h, C.byref(_query(n=0, max_depth=0, keep=keep))) == inv  # max_depth and samples are checked before n == 0
    for kw in ({}, {"rng_out": False}, {"rays": False}, {"rng_out": False, "rays": False}, {"samples": 7, "rr_start": 3}, {"max_depth": 1}):
        assert call(s.h, C.byref(_query(keep=keep, **kw))) == abi.RT_ERR_NO_DEVICE, kw
        assert "host-only" in _err(rtlib)
    assert call(s.h, C.byref(_query(n=0, keep=keep))) == abi.RT_OK
    assert call(s.h, C.byref(_query(n=0, pos=False, normal=False, rng=False, radiance=False, keep=keep))) == abi.RT_OK
    s.close()


def test_python_wrappers_refuse_wrong_shapes(rtlib):
    s = Scene(scenes.get_scene("cube"), device=-1)
    pos, nrm, rng = np.zeros((2, 3), f32), np.ones((2, 3), f32), np.ones(2, np.uint32)
    with pytest.raises(abi.RtError) as e:
        s.gather_paths(pos, nrm, rng, 5)
    assert e.value.status == abi.RT_ERR_NO_DEVICE
    for bad in ((pos, np.ones((3, 3), f32), rng), (pos, nrm, np.ones(3, np.uint32)), (pos, nrm, np.ones((2, 1), np.uint32)),
                (np.zeros(6, f32), np.ones(6, f32), rng), (np.zeros((2, 4), f32), np.ones((2, 4), f32), rng), (pos, nrm, np.ones(2, f32))):
        with pytest.raises(ValueError):
            s.gather_paths(*bad, 5)
    for kw in ({"max_depth": 0}, {"max_depth": 5, "samples": 0}):
        with pytest.raises(abi.RtError) as e:
            s.gather_paths(pos, nrm, rng, **kw)
        assert e.value.status == abi.RT_ERR_INVALID
    out = s.gather_paths(np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros(0, np.uint32), 5)
    assert out["radiance"].shape == (0, 3) and out["rng"].shape == (0,) and out["rays"].shape == (0,)
    assert out["radiance"].dtype == f32 and out["rng"].dtype == np.uint32 and out["rays"].dtype == np.uint32
    with pytest.raises(abi.RtError) as e:
        s.gather_paths_device(5, 0, 0, 0, 0, 5)
    assert e.value.status == abi.RT_ERR_INVALID
    s.close()


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
def test_unit_vector_model_equals_the_oracles_diffuse_scatter(oracle):
    """MaterialDiffuse::scatter of the oracle (an incoming direction that is not near zero): direction = normal + unit, the state three draws
    on. 4,004 states with the four special ones, normals of every kind the mix holds, zero normals included."""
    sd, osc, _ = probe_case("cornell")
    assert sd.materials[0].type == abi.RT_MAT_DIFFUSE
    g = np.random.default_rng(5)
    n = 4000
    seeds = np.concatenate([np.array([0, 1, 0x80000000, 0xFFFFFFFF], np.uint32), g.integers(1, 2**32, n, dtype=np.uint64).astype(np.uint32)])
    nrm = (g.normal(size=(n + 4, 3)) * 10.0 ** g.uniform(-2, 2, size=(n + 4, 1))).astype(f32)
    cases = np.concatenate([_directed_cases(), SPECIAL_NORMALS])
    nrm[4:4 + len(cases)] = cases
    nrm[:4] = 0.0
    d_in = np.tile(np.array([[0.6, -0.8, 0.0]], f32), (n + 4, 1))
    ok, od, _, so = osc.scatter(0, d_in, nrm, np.zeros((n + 4, 2), f32), seeds)
    u, st = unit_vector_model(seeds)
    assert ok.all()
    np.testing.assert_array_equal(od, nrm + u)
    np.testing.assert_array_equal(so, st)
    np.testing.assert_array_equal(st, steps(seeds, 3))
    assert u.dtype == f32 and st.dtype == np.uint32
    np.testing.assert_allclose(np.linalg.norm(u.astype(np.float64), axis=1), 1.0, atol=1e-6)


@pytest.mark.parametrize("name", ["cornell", "atrium", "tables"])
def test_the_point_mix_reaches_what_it_is_for(name):
    """Asserted on the oracle's gather_model, samples = 3, depth 5, with margins under what was measured when the mix was written (Cornell:
    about 83 lit entries, 77 % bounce; coarse atrium: 50 % lit, 86 % bounce; tables: 86 % lit, 53 % bounce)."""
    sd, _, (pos, nrm, state) = mix_case(name)
    samples = 3
    off, on = mix_expected(name, DEPTH, samples, 0), mix_expected(name, DEPTH, samples, 2)
    for out in (off, on):
        assert np.isfinite(out["radiance"]).all()
    lit = (off["radiance"] != 0).any(1)
    if name == "cornell":
        assert lit.sum() >= 20
    if name == "atrium":
        assert lit.mean() >= 0.20
    assert (off["rays"] > samples).mean() >= 1.0 / 3.0
    assert int(on["rays"].astype(np.uint64).sum()) < int(off["rays"].astype(np.uint64).sum())
    over = np.flatnonzero((nrm == np.array([1e5, 0.0, 0.0], f32)).all(1))
    assert len(over) >= 5
    for out in (off, on):
        assert (out["rays"][over] == samples).all()
        np.testing.assert_array_equal(out["rng"][over], steps(state[over], 3 * samples))
        np.testing.assert_array_equal(out["radiance"][over], np.tile(sky_mean(sd.sky, samples), (len(over), 1)))
    assert (state[:4] == np.array([0, 1, 0x80000000, 0xFFFFFFFF], np.uint32)).all() and len(pos) == MIX_N


def test_empty_scene_is_the_sky_after_one_ray_per_path_and_three_draws(oracle):
    sd = scenes.get_scene("empty")
    osc = oracle.OracleScene(sd)
    g = np.random.default_rng(2)
    n = 300
    pos, nrm = g.normal(size=(n, 3)).astype(f32), g.normal(size=(n, 3)).astype(f32)
    state = g.integers(1, 2**32, n, dtype=np.uint64).astype(np.uint32)
    for samples in (1, 2, 3):
        out = gather_model(osc.trace_paths, pos, nrm, state, DEPTH, samples, 0)
        np.testing.assert_array_equal(out["radiance"], np.tile(sky_mean(sd.sky, samples), (n, 1)))
        np.testing.assert_array_equal(out["rng"], steps(state, 3 * samples))
        assert (out["rays"] == samples).all()


@pytest.mark.parametrize("rr_start", [0, 2])
def test_four_samples_are_four_chained_single_sample_gathers(rr_start):
    _, osc, (pos, nrm, state) = mix_case("atrium")
    pos, nrm, state = pos[:1000], nrm[:1000], state[:1000]
    one = gather_model(osc.trace_paths, pos, nrm, state, DEPTH, 4, rr_start)
    total, rays, st = np.zeros_like(pos), np.zeros(len(pos), np.uint32), state
    for _ in range(4):
        out = gather_model(osc.trace_paths, pos, nrm, st, DEPTH, 1, rr_start)
        total, rays, st = total + out["radiance"], rays + out["rays"], out["rng"]
    np.testing.assert_array_equal(one["radiance"], total / f32(4.0))
    np.testing.assert_array_equal(one["rng"], st)
    np.testing.assert_array_equal(one["rays"], rays)
    assert rays.max() > 4


# ---- the listing --------------------------------------------------------------------------------------------------------------------------
def test_gather_kernel_passes_the_isa_hazard_scan_with_the_resources_design_states(tmp_path):
    """k_path_gather (rt_path_gather.hip) through tests/test_isa_hazards.py's checker: it carries the asm node fetch and breaks none of its
    rules. Its registers, spills, scratch, LDS and occupancy are the figures of DESIGN.md §18, read from the listing and from DESIGN.md
    itself; the occupancy is k_path_query's 6 waves per SIMD and the LDS is no more than k_path_query's."""
    from test_denoise import _listing
    from test_isa_hazards import _check
    from test_svgf import _metadata
    lines = _listing("rt_path_gather.hip", tmp_path)
    groups = _check(lines)
    assert list(groups) == [K_PATH_GATHER] and groups[K_PATH_GATHER] >= 1, groups
    meta = "\n".join(lines)
    got = {k: _metadata(meta, K_PATH_GATHER, k) for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    occ = [int(m) for m in re.findall(r"^; Occupancy: (\d+)", meta, re.M)]
    assert len(occ) == 1  # one kernel in the unit
    got["occupancy"] = occ[0]
    design = (REPO / "DESIGN.md").read_text()
    m = re.search(r"`k_path_gather`: (\d+) VGPRs, (\d+) spilled, (\d+) bytes of scratch per lane, ([\d,]+) bytes of LDS per workgroup, (\d+) waves per SIMD", design)
    assert m, "DESIGN.md states k_path_gather's resources in one sentence"
    stated = {"vgpr_count": int(m.group(1)), "vgpr_spill_count": int(m.group(2)), "private_segment_fixed_size": int(m.group(3)),
              "group_segment_fixed_size": int(m.group(4).replace(",", "")), "occupancy": int(m.group(5))}
    assert got == stated
    assert got["occupancy"] == 6 and got["vgpr_count"] <= 80  # 6 waves per SIMD (512 registers / 6, in blocks of 8)
    assert 3 * got["group_segment_fixed_size"] <= 160 * 1024  # three 512-thread workgroups per CU: 24 waves = 6 per SIMD
    pq = "\n".join(_listing("rt_path_query.hip", tmp_path))
    assert got["group_segment_fixed_size"] <= _metadata(pq, K_PATH_QUERY, "group_segment_fixed_size")


# ---- the baker's points --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "tables"])
def test_vertex_points_are_the_world_triangles_with_unit_normals(name):
    sd = probe_case(name)[0]
    pos, nrm = bake.vertex_points(sd)
    tw = sd.world_triangles()
    assert pos.shape == nrm.shape == tw.shape == (sd.n_triangles, 3, 3) and pos.dtype == f32 and nrm.dtype == f32
    scale = np.abs(tw).max()
    np.testing.assert_allclose(pos, tw, rtol=0, atol=4 * 2.0**-24 * scale)  # three products and three sums of terms bounded by the scale
    np.testing.assert_allclose(np.linalg.norm(nrm.astype(np.float64), axis=2), 1.0, atol=1e-6)
    if name == "cornell":  # every corner's normal lies on the face's side (the winding's); on the flat-shaded walls and boxes it is the face's
        face = np.cross(tw[:, 1] - tw[:, 0], tw[:, 2] - tw[:, 0])
        face /= np.linalg.norm(face, axis=1, keepdims=True)
        cos = np.einsum("tcj,tj->tc", nrm.astype(np.float64), face)
        assert (cos > 0).all()
        flat = (np.abs(nrm - nrm[:, :1]).max(axis=(1, 2)) < 1e-6)  # the triangles whose three corners share one normal
        assert flat.sum() >= 12 and (cos[flat] > 1.0 - 1e-5).all()


def test_corner_seeds_are_distinct_and_never_zero():
    s = bake.corner_seeds(1000, 3, 7)
    assert s.shape == (1000, 3) and s.dtype == np.uint32 and (s != 0).all() and len(np.unique(s)) == 3000
    assert not np.array_equal(s, bake.corner_seeds(1000, 3, 8))
