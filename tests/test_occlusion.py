"""Occlusion gathers (include/rt_mi355x.h: rt_gather_occlusion[_device], rt_scene_occlusion_host) without a GPU: the exported entry points
and the struct layout, the refusals in front of the device, the Python wrappers' refusals, the host diagnostic — brute force and the
kernel's walk — against the numpy model over the oracle's brute force (tests/occlusion_scenes.py), the contract's corners, the conditions
on the tests' inputs, the baker, and the listing of the kernel's unit (ISA hazard scan, resources as DESIGN.md §26 states them). Every
comparison is bit for bit."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import occlusion_scenes as oc
from occlusion_scenes import OUTPUTS, mix_case, mix_expected, occlusion_model, oracle_occluder, same, steps
from rtamd import abi, bake, scenes
from rtamd.renderer import Scene
from test_closest_points import tri_scene
from test_gather import unit_vector_model

REPO = Path(__file__).resolve().parent.parent
f32 = np.float32
K_OCCLUSION = "_ZN2rt18k_occlusion_gatherENS_8SceneDevENS_12OcclusionDevE"
K_QUERY_ANY = "_ZN2rt7k_queryILb1EEEvNS_8SceneDevENS_8QueryDevE"
FIELDS = ["n", "samples", "pos", "normal", "max_dist", "rng", "rng_out", "visibility", "bent", "clear", "rays"]


# ---- the surface --------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_prototyped(rtlib, devlib, tmp_path):
    for lib in (rtlib, devlib):  # (first: on a tree without the feature the test ends here, at the symbol lookup)
        for name in ("rt_gather_occlusion", "rt_gather_occlusion_device", "rt_scene_occlusion_host"):
            assert hasattr(lib, name), name
    header = (REPO / "include" / "rt_mi355x.h").read_text()
    assert "typedef struct rt_occlusion_query {" in header and "#define RT_OCCLUSION_MAX_SAMPLES 65535" in header
    assert abi.RT_OCCLUSION_MAX_SAMPLES == 65535
    for name in ("rt_gather_occlusion", "rt_gather_occlusion_device"):
        assert re.search(rf"^int {name}\(rt_scene\* scene, const rt_occlusion_query\* q", header, re.M), name
        assert name in abi.PROTOTYPES
    assert re.search(r"^int rt_scene_occlusion_host\(const rt_scene\* scene, const rt_occlusion_query\* q, int use_bvh", header, re.M)
    assert "rt_scene_occlusion_host" in abi.PROTOTYPES
    assert [f[0] for f in abi.rt_occlusion_query._fields_] == FIELDS
    assert rtlib.rt_abi_version() == 8 and "#define RT_ABI_VERSION 8" in header
    # the layout, measured by compiling a C program against the header
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_mi355x.h"\nint main(void){printf("%zu\\n", sizeof(rt_occlusion_query));' +
                   "".join(f'printf("%zu\\n", offsetof(rt_occlusion_query, {f}));' for f in FIELDS) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", str(REPO / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(abi.rt_occlusion_query)] + [getattr(abi.rt_occlusion_query, f).offset for f in FIELDS]
    assert got[0] == 80


def _query(n=4, samples=3, keep=None, **null):
    bufs = {"pos": np.zeros((4, 3), f32), "normal": np.ones((4, 3), f32), "max_dist": np.ones(4, f32), "rng": np.arange(1, 5, dtype=np.uint32),
            "rng_out": np.zeros(4, np.uint32), "visibility": np.zeros(4, f32), "bent": np.zeros((4, 3), f32), "clear": np.zeros(4, np.uint32),
            "rays": np.zeros(4, np.uint32)}
    if keep is not None:
        keep.append(bufs)
    q = abi.rt_occlusion_query(n=n, samples=samples)
    for name, a in bufs.items():
        setattr(q, name, a.ctypes.data if null.get(name, True) else None)
    return q


def _err(lib):
    return lib.rt_last_error().decode()


@pytest.mark.parametrize("entry", ["rt_gather_occlusion", "rt_gather_occlusion_device"])
def test_refusals_come_in_order_before_any_device_call(rtlib, entry):
    """On a host-only scene no device call can succeed, so every status below was decided in front of the device, in the header's order: a
    NULL scene or query; n == 0 is RT_OK whatever else the query holds; samples; NULL pos, normal or rng; every output NULL;
    RT_ERR_NO_DEVICE last."""
    s = Scene(scenes.get_scene("cornell"), device=-1)
    fn = getattr(rtlib, entry)
    call = (lambda h, q: fn(h, q)) if entry == "rt_gather_occlusion" else (lambda h, q: fn(h, q, None))
    keep = []
    inv = abi.RT_ERR_INVALID
    outs = {"visibility": False, "bent": False, "clear": False, "rays": False}
    assert call(None, C.byref(_query(keep=keep))) == inv and "null argument" in _err(rtlib)
    assert call(s.h, None) == inv and "null argument" in _err(rtlib)
    assert call(None, C.byref(_query(n=0, keep=keep))) == inv  # the NULL scene comes before n == 0
    assert call(s.h, C.byref(_query(n=0, samples=0, pos=False, normal=False, rng=False, keep=keep, **outs))) == abi.RT_OK  # n == 0 before the rest
    for kw, word in (({"samples": 0}, "samples"), ({"samples": 65536}, "samples"), ({"samples": 0xFFFFFFFF}, "samples"), ({"pos": False}, "pos"),
                     ({"normal": False}, "normal"), ({"rng": False}, "rng"), (outs, "every output NULL")):
        assert call(s.h, C.byref(_query(keep=keep, **kw))) == inv, kw
        assert word in _err(rtlib), (kw, _err(rtlib))
    assert call(s.h, C.byref(_query(samples=0, pos=False, keep=keep))) == inv and "samples" in _err(rtlib)  # samples before the pointers
    assert call(s.h, C.byref(_query(rng=False, keep=keep, **outs))) == inv and "rng" in _err(rtlib)         # the inputs before the outputs
    for kw in ({}, {"max_dist": False}, {"rng_out": False}, {"samples": 65535}, {"visibility": False, "bent": False, "clear": False},
               {"bent": False, "clear": False, "rays": False}):
        assert call(s.h, C.byref(_query(keep=keep, **kw))) == abi.RT_ERR_NO_DEVICE, kw
        assert "host-only" in _err(rtlib)
    s.close()


def test_python_wrappers_refuse_wrong_shapes_and_dtypes(rtlib):
    s = Scene(scenes.get_scene("cube"), device=-1)
    pos, nrm, rng = np.zeros((2, 3), f32), np.ones((2, 3), f32), np.ones(2, np.uint32)
    with pytest.raises(abi.RtError) as e:
        s.gather_occlusion(pos, nrm, rng, 4)
    assert e.value.status == abi.RT_ERR_NO_DEVICE
    for fn in (s.gather_occlusion, s.occlusion_host):
        for bad in ((pos, np.ones((3, 3), f32), rng), (pos, nrm, np.ones(3, np.uint32)), (pos, nrm, np.ones((2, 1), np.uint32)),
                    (np.zeros(6, f32), np.ones(6, f32), rng), (np.zeros((2, 4), f32), np.ones((2, 4), f32), rng), (pos, nrm, np.ones(2, f32))):
            with pytest.raises(ValueError):
                fn(*bad, 4)
        for md in (np.ones(3, f32), np.ones((2, 1), f32), np.array(["a", "b"]), "far"):
            with pytest.raises(ValueError):
                fn(pos, nrm, rng, 4, md)
        for samples in (2.0, True, None):
            with pytest.raises(ValueError):
                fn(pos, nrm, rng, samples)
        for samples in (0, 65536):
            with pytest.raises(abi.RtError) as e:
                fn(pos, nrm, rng, samples)
            assert e.value.status == abi.RT_ERR_INVALID
    out = s.gather_occlusion(np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros(0, np.uint32), 4)
    assert out["visibility"].shape == (0,) and out["bent"].shape == (0, 3) and out["clear"].shape == out["rays"].shape == out["rng"].shape == (0,)
    assert out["visibility"].dtype == out["bent"].dtype == f32 and out["clear"].dtype == out["rays"].dtype == out["rng"].dtype == np.uint32
    with pytest.raises(abi.RtError) as e:
        s.gather_occlusion_device(5, 0, 0, 0, 4)
    assert e.value.status == abi.RT_ERR_INVALID
    keep = []
    assert rtlib.rt_scene_occlusion_host(s.h, C.byref(_query(keep=keep)), 2, None, None) == abi.RT_ERR_INVALID and "use_bvh" in _err(rtlib)
    assert rtlib.rt_scene_occlusion_host(s.h, C.byref(_query(keep=keep, rng=False)), 0, None, None) == abi.RT_ERR_INVALID
    assert rtlib.rt_scene_occlusion_host(None, C.byref(_query(keep=keep)), 0, None, None) == abi.RT_ERR_INVALID
    h = s.occlusion_host(pos, nrm, rng, 4, 1.5)  # one distance for every entry; an integer array of states
    same(s.occlusion_host(pos, nrm, rng.astype(np.int64), 4, np.full(2, 1.5)), h, "broadcast radius")
    s.close()


# ---- the conditions on the inputs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", oc.SCENES)
def test_the_entries_and_radii_reach_what_they_are_for(name):
    """Conditions, checked with the model over the oracle's brute force at samples = 7 under the radius mix: between 10 % and 90 % of the
    traced samples are occluded, at least 5 % of the entries are fully clear and at least 5 % fully occluded. (Measured when the mix was
    written, occluded / fully clear / fully occluded: Cornell 34 % / 57 % / 23 %, coarse atrium 48 % / 43 % / 33 % on its 129 entries,
    tables 33 % / 53 % / 21 %.) The mix holds every radius kind, the all-degenerate entries and the entry whose first sample has l2 == 0."""
    c = mix_case(name)
    samples = 7
    m = mix_expected(name, samples, True)
    traced = int(m["rays"].sum())
    occluded = int((samples - m["clear"].astype(np.int64)).sum())
    share, clear, dark = occluded / traced, (m["clear"] == samples).mean(), (m["clear"] == 0).mean()
    print(f"{name}: {share:.3f} of the traced samples occluded, {clear:.3f} of the entries fully clear, {dark:.3f} fully occluded")
    assert 0.10 <= share <= 0.90 and clear >= 0.05 and dark >= 0.05
    r = c["radii"]
    for v in (-1.0, 0.0):
        assert (r == f32(v)).any()
    assert (np.signbit(r) & (r == 0)).any() and np.isposinf(r).any() and ((r > 0) & np.isfinite(r)).sum() >= len(r) // 4
    assert (m["rays"][c["degenerate"]] == 0).all() and len(c["degenerate"]) == 8
    assert m["rays"][12] == samples - 1  # the l2 == 0 entry: one sample without a ray


# ---- the host diagnostic against the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", oc.SCENES)
def test_brute_force_and_walk_equal_the_model_over_the_oracle(rtlib, name):
    """rt_scene_occlusion_host, use_bvh = 0 and 1, against occlusion_model over OracleScene.intersect(use_bvh=False): samples = 1, 2, 7 and
    64, free (max_dist NULL) and under the radius mix. On the coarse atrium (235,750 triangles under two brute forces) samples = 64 runs on
    the first 33 entries."""
    c = mix_case(name)
    s = Scene(c["sd"], device=-1)
    for samples in (1, 2, 7, 64):
        n = 33 if (name == "atrium" and samples == 64) else len(c["pos"])
        for mixed in (False, True):
            want = mix_expected(name, samples, mixed, None if n == len(c["pos"]) else n)
            md = c["radii"][:n] if mixed else None
            what = f"{name} samples={samples}{' mix' if mixed else ''}"
            walk = s.occlusion_host(c["pos"][:n], c["nrm"][:n], c["state"][:n], samples, md, use_bvh=True)
            same(walk, want, what + ": walk")
            same(s.occlusion_host(c["pos"][:n], c["nrm"][:n], c["state"][:n], samples, md), want, what + ": brute force")
            assert walk["node_visits"] > 0
    s.close()


def test_null_max_dist_is_plus_infinity_and_outputs_may_be_null(rtlib):
    c = mix_case("cornell")
    s = Scene(c["sd"], device=-1)
    n = 200
    free = s.occlusion_host(c["pos"][:n], c["nrm"][:n], c["state"][:n], 5)
    same(s.occlusion_host(c["pos"][:n], c["nrm"][:n], c["state"][:n], 5, np.full(n, np.inf, f32)), free, "+inf")
    pos, nrm, st = (c[k][:n].copy() for k in ("pos", "nrm", "state"))  # copies: rng_out == rng below writes into st
    vis = np.full(n, 7, f32)
    q = abi.rt_occlusion_query(n=n, samples=5, pos=pos.ctypes.data, normal=nrm.ctypes.data, rng=st.ctypes.data, visibility=vis.ctypes.data)
    abi.check(rtlib.rt_scene_occlusion_host(s.h, C.byref(q), 1, None, None), rtlib)
    np.testing.assert_array_equal(vis, free["visibility"])
    q.rng_out = st.ctypes.data  # rng_out == rng
    abi.check(rtlib.rt_scene_occlusion_host(s.h, C.byref(q), 0, None, None), rtlib)
    np.testing.assert_array_equal(st, free["rng"])
    s.close()


def test_four_samples_are_four_chained_single_sample_gathers(rtlib):
    c = mix_case("tables")
    s = Scene(c["sd"], device=-1)
    pos, nrm, md = c["pos"], c["nrm"], c["radii"]
    for bvh in (False, True):
        one = s.occlusion_host(pos, nrm, c["state"], 4, md, use_bvh=bvh)
        st, clear, rays, parts = c["state"], np.zeros(len(pos), np.uint32), np.zeros(len(pos), np.uint32), []
        for _ in range(4):
            out = s.occlusion_host(pos, nrm, st, 1, md, use_bvh=bvh)
            st, clear, rays = out["rng"], clear + out["clear"], rays + out["rays"]
            parts.append(out["bent"])
        np.testing.assert_array_equal(one["clear"], clear)
        np.testing.assert_array_equal(one["rays"], rays)
        np.testing.assert_array_equal(one["rng"], st)
        np.testing.assert_array_equal(one["bent"], (((parts[0] + parts[1]) + parts[2]) + parts[3]) / f32(4.0))
        np.testing.assert_array_equal(one["visibility"], clear.astype(f32) / f32(4.0))
    assert 0 < clear.sum() < 4 * len(pos) and rays.max() == 4
    s.close()


def test_degenerate_entries_trace_nothing_and_still_draw(rtlib):
    """Normals of 1e20: l2 overflows on every sample — rays = 0, visibility = 1, bent = 0, the state 3 x samples draws on. The entry whose
    normal is the negative of its first unit vector has l2 == 0 on that sample alone."""
    c = mix_case("cornell")
    s = Scene(c["sd"], device=-1)
    at = c["degenerate"]
    for samples in (1, 7, 64):
        for bvh in (False, True):
            out = s.occlusion_host(c["pos"], c["nrm"], c["state"], samples, c["radii"], use_bvh=bvh)
            assert (out["rays"][at] == 0).all() and (out["clear"][at] == samples).all() and (out["visibility"][at] == 1).all()
            assert not out["bent"][at].any() and not np.signbit(out["bent"][at]).any()
            np.testing.assert_array_equal(out["rng"], steps(c["state"], 3 * samples))  # every entry: the draws do not depend on what is hit
            assert out["rays"][12] == samples - 1
    s.close()


def test_the_empty_scene_and_the_single_triangle(rtlib, oracle):
    g = np.random.default_rng(2)
    n = 300
    pos, nrm = g.normal(size=(n, 3)).astype(f32), g.normal(size=(n, 3)).astype(f32)
    state = g.integers(1, 2**32, n, dtype=np.uint64).astype(np.uint32)
    s = Scene(scenes.get_scene("empty"), device=-1)
    for samples in (1, 3, 16):
        total, st = np.zeros((n, 3), f32), state
        for _ in range(samples):  # the ordered mean of the directions
            u, st = unit_vector_model(st)
            d = nrm + u
            total = total + d * (f32(1.0) / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))[:, None]
        for bvh in (False, True):
            out = s.occlusion_host(pos, nrm, state, samples, use_bvh=bvh)
            assert (out["clear"] == samples).all() and (out["rays"] == samples).all() and (out["visibility"] == 1).all()
            np.testing.assert_array_equal(out["bent"], total / f32(samples))
            np.testing.assert_array_equal(out["rng"], st)
    s.close()
    tri = np.array([[[-1.0, -1.0, 1.0], [1.0, -1.0, 1.0], [0.0, 1.5, 1.0]]], f32)
    sd = tri_scene("one", tri)
    s = Scene(sd, device=-1)
    pos = (g.uniform(-0.3, 0.3, (n, 3)) * np.array([1, 1, 0.5])).astype(f32)
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]], f32), (n, 1))
    want = occlusion_model(oracle_occluder(oracle.OracleScene(sd)), pos, nrm, state, 8)
    assert 0.2 < 1.0 - want["visibility"].mean() < 0.95
    for bvh in (False, True):
        same(s.occlusion_host(pos, nrm, state, 8, use_bvh=bvh), want, f"single triangle bvh={bvh}")
    s.close()


def test_max_dist_on_a_hits_t_occludes_and_the_next_float_below_does_not(rtlib, oracle):
    c = mix_case("cornell")
    pos, nrm, state = c["pos"], c["nrm"], c["state"]
    u, _ = unit_vector_model(state)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        d = nrm + u
        l2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        w = d * (f32(1.0) / np.sqrt(l2))[:, None]
    ok = (l2 > 0) & np.isfinite(l2)
    t, _, _, tri = c["osc"].intersect(pos[ok], np.ascontiguousarray(w[ok]), False)
    hit = np.flatnonzero(ok)[(tri != 0xFFFFFFFF) & np.isfinite(t)]
    t = t[(tri != 0xFFFFFFFF) & np.isfinite(t)]
    assert len(hit) > 300
    s = Scene(c["sd"], device=-1)
    for bvh in (False, True):
        on = s.occlusion_host(pos[hit], nrm[hit], state[hit], 1, t, use_bvh=bvh)
        below = s.occlusion_host(pos[hit], nrm[hit], state[hit], 1, np.nextafter(t, f32(-np.inf)), use_bvh=bvh)
        assert (on["clear"] == 0).all() and (on["visibility"] == 0).all() and not on["bent"].any()
        assert (below["clear"] == 1).all() and (below["rays"] == 1).all()
        np.testing.assert_array_equal(below["bent"], w[hit])
    s.close()


def _walk_scenes():
    from test_scene_update import chain_scene
    return {
        "atrium_sah": lambda lib: Scene(scenes.get_scene("atrium", detail=1), -1, abi.RT_BVH_SAH, lib=lib),
        "atrium_lbvh": lambda lib: Scene(scenes.get_scene("atrium", detail=1), -1, abi.RT_BVH_LBVH, lib=lib),
        "median": lambda lib: Scene(chain_scene(), -1, abi.RT_BVH_LBVH, lib=lib),
        "cornell_lbvh": lambda lib: Scene(scenes.get_scene("cornell"), -1, abi.RT_BVH_LBVH, lib=lib),
    }


@pytest.mark.parametrize("case", ["atrium_sah", "atrium_lbvh", "median", "cornell_lbvh"])
def test_the_walk_equals_the_brute_force_on_every_builder(devlib, case):
    """use_bvh = 1 == use_bvh = 0 bit for bit under SAH, LBVH and the median fallback, free and under the radius mix; with a radius the walk
    visits fewer nodes than without."""
    from test_path_query import scene_bounds
    s = _walk_scenes()[case](devlib)
    assert s.tree()["built_by"] == {"atrium_sah": abi.RT_BVH_SAH, "median": abi.RT_BVH_MEDIAN_INTERNAL}.get(case, abi.RT_BVH_LBVH)
    n = 512
    pos, nrm, state, _ = oc.entries(s.desc, n, 11)
    radii = oc.radius_mix(n, scene_bounds(s.desc)[2], 5)
    if case == "median":  # half of the lobes narrowed onto the corner cell of the forty-one equal triangles (nothing else is large enough to meet)
        to = np.random.default_rng(5).uniform(0.0, 2.0 ** -23, (n // 2, 3)) - pos[n // 2:].astype(np.float64)
        nrm[n // 2:] = (to * (1e8 / np.linalg.norm(to, axis=1, keepdims=True))).astype(f32)
        radii[n // 2:] = np.where(radii[n // 2:] > 0, f32(np.inf), radii[n // 2:])
    visits = {}
    for name, md in (("free", None), ("mix", radii)):
        for samples in (1, 5):
            walk = s.occlusion_host(pos, nrm, state, samples, md, use_bvh=True)
            same(walk, s.occlusion_host(pos, nrm, state, samples, md), f"{case} {name} samples={samples}")
            visits[name, samples] = walk["node_visits"]
            if name == "free":
                assert 0 < walk["clear"].sum() < samples * n or (case == "median" and samples == 1), (case, samples)  # some occluded, some clear
    assert visits["mix", 5] < visits["free", 5] and visits["mix", 1] < visits["free", 1]
    s.close()


def test_the_sample_limit(rtlib):
    s = Scene(scenes.get_scene("empty"), device=-1)
    pos, nrm, state = np.zeros((1, 3), f32), np.array([[0.0, 0.0, 1.0]], f32), np.array([12345], np.uint32)
    out = s.occlusion_host(pos, nrm, state, 65535, use_bvh=True)
    assert out["clear"][0] == out["rays"][0] == 65535 and out["visibility"][0] == 1
    np.testing.assert_array_equal(out["rng"], steps(state, 3 * 65535))
    assert 0.5 < out["bent"][0, 2] <= 1.0
    with pytest.raises(abi.RtError) as e:
        s.occlusion_host(pos, nrm, state, 65536)
    assert e.value.status == abi.RT_ERR_INVALID and "samples" in str(e.value)
    s.close()


# ---- the baker ---------------------------------------------------------------------------------------------------------------------------------
class _HostGather:
    """a Scene whose gather_occlusion is the host diagnostic's: what bake_vertex_ao calls, without a device"""
    def __init__(self, scene):
        self.scene = scene

    def gather_occlusion(self, pos, nrm, rng, samples, max_dist=None):
        return self.scene.occlusion_host(pos, nrm, rng, samples, max_dist, use_bvh=True)


def test_bake_vertex_ao_equals_the_wrapper_on_vertex_points(rtlib):
    sd = scenes.get_scene("cornell")
    s = Scene(sd, device=-1)
    pos, nrm = bake.vertex_points(sd)
    c = sd.n_triangles * 3
    for repeats in (1, 3):
        vis, bent = bake.bake_vertex_ao(_HostGather(s), sd, 6, 0.5, 9, repeats=repeats)
        assert vis.shape == (sd.n_triangles, 3) and bent.shape == (sd.n_triangles, 3, 3) and vis.dtype == bent.dtype == f32
        out = s.occlusion_host(np.repeat(pos.reshape(c, 3), repeats, axis=0), np.repeat(nrm.reshape(c, 3), repeats, axis=0),
                               bake.corner_seeds(c, repeats, 9).reshape(-1), 6, 0.5, use_bvh=True)
        tv, tb = np.zeros(c, f32), np.zeros((c, 3), f32)
        for k in range(repeats):
            tv, tb = tv + out["visibility"].reshape(c, repeats)[:, k], tb + out["bent"].reshape(c, repeats, 3)[:, k]
        np.testing.assert_array_equal(vis.reshape(-1), tv / f32(repeats))
        np.testing.assert_array_equal(bent.reshape(-1, 3), bake.normalise_bent(tb / f32(repeats)))
        assert 0.1 < vis.mean() < 0.95
    with pytest.raises(ValueError):
        bake.bake_vertex_ao(_HostGather(s), sd, 6, 0.5, 9, repeats=0)
    s.close()


def test_normalise_bent_is_zero_where_bent_is_zero():
    b = np.array([[0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [0.0, 0.0, 0.25], [3.0, -4.0, 0.0]], f32)
    out = bake.normalise_bent(b)
    assert out.dtype == f32 and not out[:2].any()
    np.testing.assert_array_equal(out[2:], np.array([[0.0, 0.0, 1.0], [f32(3.0) * (f32(1.0) / f32(5.0)), f32(-4.0) * (f32(1.0) / f32(5.0)), 0.0]], f32))
    assert bake.normalise_bent(np.zeros((2, 3, 3), f32)).shape == (2, 3, 3)
    with pytest.raises(ValueError):
        bake.normalise_bent(np.zeros((2, 2), f32))


# ---- the listing ----------------------------------------------------------------------------------------------------------------------------
def test_the_kernel_passes_the_isa_hazard_scan_with_the_resources_design_states(tmp_path):
    """k_occlusion_gather (rt_occlusion.hip) through tests/test_isa_hazards.py's checker: it carries the asm node fetch and breaks none of
    its rules. No VGPR is spilled, its scratch is k_query<true>'s stack frame, and its registers, LDS and occupancy are the figures of
    DESIGN.md §26, read from the listing and from DESIGN.md itself."""
    from test_denoise import _listing
    from test_isa_hazards import _check
    from test_svgf import _metadata
    lines = _listing("rt_occlusion.hip", tmp_path)
    groups = _check(lines)
    assert list(groups) == [K_OCCLUSION] and groups[K_OCCLUSION] >= 1, groups
    meta = "\n".join(lines)
    got = {k: _metadata(meta, K_OCCLUSION, k) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    occ = [int(m) for m in re.findall(r"^; Occupancy: (\d+)", meta, re.M)]
    assert len(occ) == 1  # one kernel in the unit
    got["occupancy"] = occ[0]
    design = (REPO / "DESIGN.md").read_text()
    m = re.search(r"`k_occlusion_gather`: (\d+) VGPRs, (\d+) spilled, (\d+) SGPRs, (\d+) bytes of scratch per lane, ([\d,]+) bytes of LDS per workgroup, (\d+) waves per SIMD", design)
    assert m, "DESIGN.md states k_occlusion_gather's resources in one sentence"
    stated = {"vgpr_count": int(m.group(1)), "vgpr_spill_count": int(m.group(2)), "sgpr_count": int(m.group(3)), "private_segment_fixed_size": int(m.group(4)),
              "group_segment_fixed_size": int(m.group(5).replace(",", "")), "occupancy": int(m.group(6))}
    assert got == stated
    assert got["vgpr_spill_count"] == 0 and _metadata(meta, K_OCCLUSION, "sgpr_spill_count") == 0
    rq = "\n".join(_listing("rt_query.hip", tmp_path))
    assert got["private_segment_fixed_size"] == _metadata(rq, K_QUERY_ANY, "private_segment_fixed_size") == 224
    assert got["group_segment_fixed_size"] == _metadata(rq, K_QUERY_ANY, "group_segment_fixed_size")
    assert got["occupancy"] == 6 and got["vgpr_count"] <= 80  # 6 waves per SIMD (512 registers / 6, in blocks of 8)
