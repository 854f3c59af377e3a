"""Closest-point queries (include/rt_mi355x.h: rt_closest_points[_device], rt_scene_closest_host) without a GPU: the exported entry points
and the struct layout, the refusals in front of the device, the Python wrappers, the numpy model of the contract (closest_model, shared
with tests/test_gpu_closest_points.py) against the host brute force, ties, degenerate triangles and radii on the boundary, the underestimate
bound the cull leans on, and the host walk of the tree (the kernel's cull rule) against the brute force on every builder — and, at the
end, on the scenes of tests/closest_scenes.py, the trees tests/test_gpu_closest_points_trees.py holds the kernel's own steps on."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rtamd import abi, bake, scenes
from rtamd.renderer import Scene

REPO = Path(__file__).resolve().parent.parent
f32 = np.float32
NO_TRI = 0xFFFFFFFF
OUTPUTS = ("dist2", "u", "v", "tri", "point")


# ---- the model both files share ---------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def closest_candidates(p, v0, e1, e2):
    """The contract's text (csrc/rt_closest_point.h) in numpy fp32 on broadcastable (.., 3) float32 arrays: every operation one fp32
    operation as bracketed, the regions by np.where in REVERSE order so that the first that holds wins. -> (dist2, u, v, r)"""
    for a in (p, v0, e1, e2):
        assert a.dtype == f32
    with np.errstate(all="ignore"):
        ap = p - v0
        d1, d2 = _dot(e1, ap), _dot(e2, ap)
        bp = ap - e1
        d3, d4 = _dot(e1, bp), _dot(e2, bp)
        cp = ap - e2
        d5, d6 = _dot(e1, cp), _dot(e2, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        den = (va + vb) + vc
        u, v = vb / den, vc / den
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        m = (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)
        u, v = np.where(m, f32(1.0) - w, u), np.where(m, w, v)
        m = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        u, v = np.where(m, zero, u), np.where(m, d2 / (d2 - d6), v)
        m = (d6 >= 0) & (d5 <= d6)
        u, v = np.where(m, zero, u), np.where(m, one, v)
        m = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        u, v = np.where(m, d1 / (d1 - d3), u), np.where(m, zero, v)
        m = (d3 >= 0) & (d4 <= d3)
        u, v = np.where(m, one, u), np.where(m, zero, v)
        m = (d1 <= 0) & (d2 <= 0)
        u, v = np.where(m, zero, u), np.where(m, zero, v)
        r = (ap - u[..., None] * e1) - v[..., None] * e2
        dist2 = _dot(r, r)
    assert dist2.dtype == f32 and u.dtype == f32 and r.dtype == f32
    return dist2, u, v, r


def closest_model(pos, wverts, max_dist2=None):
    """The query by brute force: pos (n, 3) float32, wverts (T, 3, 3) float32 world vertices in global order (the record is v0, v1 - v0,
    v2 - v0 in fp32), max_dist2 (n,) or None. The winner rule in index order: a candidate wins iff dist2 < best or dist2 == best at a
    lower index — in ascending index order that is dist2 < best, or dist2 == best while nothing has won. -> dict of OUTPUTS"""
    pos = np.ascontiguousarray(pos, f32)
    n = len(pos)
    best = np.full(n, np.inf, f32) if max_dist2 is None else np.array(max_dist2, f32, copy=True)
    tri = np.full(n, NO_TRI, np.uint32)
    u, v, r = np.zeros(n, f32), np.zeros(n, f32), np.zeros((n, 3), f32)
    for t, w in enumerate(np.asarray(wverts, f32).reshape(-1, 3, 3)):
        d2, cu, cv, cr = closest_candidates(pos, w[0][None], (w[1] - w[0])[None], (w[2] - w[0])[None])
        with np.errstate(invalid="ignore"):
            win = (d2 < best) | ((d2 == best) & (tri == NO_TRI))
        best, tri = np.where(win, d2, best), np.where(win, np.uint32(t), tri)
        u, v, r = np.where(win, cu, u), np.where(win, cv, v), np.where(win[:, None], cr, r)
    hit = tri != NO_TRI
    return {"dist2": np.where(hit, best, f32(np.inf)), "u": u, "v": v, "tri": tri,
            "point": np.where(hit[:, None], pos - r, f32(np.nan))}


def same(a, b, what=""):
    """bit for bit, NaNs included, on every output"""
    for k in OUTPUTS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
        bad = np.flatnonzero((x.view(np.uint32) != y.view(np.uint32)).reshape(len(x), -1).any(1))
        assert bad.size == 0, f"{what}: {k} differs at {bad.size} entries, first {bad[0]}: {x[bad[0]]} vs {y[bad[0]]}"


def bounds_of(sd):
    """(lo, hi, scale): the bounds of the world triangles and the contract's scene scale; the unit cube's for a scene without triangles"""
    v = np.asarray(sd.world_triangles(), np.float64).reshape(-1, 3)
    if len(v) == 0:
        return np.zeros(3), np.ones(3), 1.0
    lo, hi = v.min(0), v.max(0)
    return lo, hi, float(max((hi - lo).max(), np.abs(lo).max(), np.abs(hi).max()))


def point_mix(sd, n, seed, far=1.0 / 3.0):
    """Points a caller sends, shuffled, (n, 3) float32: a share `far` of them 50 to 100 scene scales outside the bounds on one to three
    axes; of the rest a quarter each uniform inside the bounds, up to half an extent outside on every side, ON the surface (vertices, edge
    points, triangle centres, random barycentrics: fp32 roundings of them) and 1e-3 scales off the surface."""
    g = np.random.default_rng(seed)
    lo, hi, scale = bounds_of(sd)
    ext = np.maximum(hi - lo, 1e-3 * scale)
    tw = np.asarray(sd.world_triangles(), np.float64).reshape(-1, 3, 3)
    n_far = int(n * far)
    n_near = n - n_far
    parts = []
    k = n_near // 4
    parts.append(g.uniform(lo, hi, (k, 3)))
    parts.append(lo - 0.5 * ext + g.uniform(0, 1, (k, 3)) * 2.0 * ext)
    if len(tw):
        t = tw[g.integers(0, len(tw), k)]
        kind = g.integers(0, 4, k)
        bu, bv = g.uniform(size=k), g.uniform(size=k)
        fold = bu + bv > 1
        bu, bv = np.where(fold, 1 - bu, bu), np.where(fold, 1 - bv, bv)
        corner = g.integers(0, 3, k)
        bu = np.where(kind == 0, (corner == 1) * 1.0, np.where(kind == 1, bu, np.where(kind == 2, 1.0 / 3.0, bu)))
        bv = np.where(kind == 0, (corner == 2) * 1.0, np.where(kind == 1, 0.0, np.where(kind == 2, 1.0 / 3.0, bv)))
        surf = t[:, 0] + bu[:, None] * (t[:, 1] - t[:, 0]) + bv[:, None] * (t[:, 2] - t[:, 0])
        parts.append(surf)
        k2 = n_near - 3 * k
        t = tw[g.integers(0, len(tw), k2)]
        off = g.normal(size=(k2, 3))
        parts.append(t.mean(1) + 1e-3 * scale * off / np.linalg.norm(off, axis=1, keepdims=True))
    else:
        parts.append(g.normal(size=(n_near - 2 * k, 3)))
    o = g.uniform(lo, hi, (n_far, 3))
    axes = g.integers(1, 8, n_far)
    out = g.uniform(50.0, 100.0, (n_far, 3)) * scale
    below = g.integers(0, 2, (n_far, 3)) == 1
    parts.append(np.where((axes[:, None] >> np.arange(3)) & 1 == 1, np.where(below, lo - out, hi + out), o))
    pos = np.concatenate(parts).astype(f32)
    assert len(pos) == n
    return np.ascontiguousarray(pos[g.permutation(n)])


def tri_scene(name, tris):
    """One instance, identity transform (world vertices = positions), one diffuse material."""
    tris = np.asarray(tris, f32).reshape(-1, 3, 3)
    sb = scenes.SceneBuilder(name)
    m = sb.add_material(scenes.Material(abi.RT_MAT_DIFFUSE, (0.6, 0.5, 0.4)))
    pos = tris.reshape(-1, 3)
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]], f32), (len(pos), 1))
    sb.add_instance(sb.add_mesh(pos, nrm, np.zeros((len(pos), 2), f32), np.arange(len(pos), dtype=np.uint32)), m)
    sb.camera = scenes.CameraPose((0.3, 0.4, 2.5), (-0.3, -0.4, -2.5), 1.2)
    return sb.build()


def world_vertices(sd):
    """the fp32 world vertices as the scene builder computes them, (T, 3, 3)"""
    return bake.vertex_points(sd)[0]


# ---- the surface --------------------------------------------------------------------------------------------------------------------------
FIELDS = ["n", "pos", "max_dist2", "dist2", "u", "v", "tri", "point"]


def test_entry_points_are_declared_exported_and_prototyped(rtlib, devlib, tmp_path):
    header = (REPO / "include" / "rt_mi355x.h").read_text()
    assert "typedef struct rt_point_query {" in header
    for name in ("rt_closest_points", "rt_closest_points_device"):
        assert re.search(rf"^int {name}\(rt_scene\* scene, const rt_point_query\* q", header, re.M), name
    assert re.search(r"^int rt_scene_closest_host\(const rt_scene\* scene, uint32_t n, const float\* pos, const float\* max_dist2, int use_bvh", header, re.M)
    for name in ("rt_closest_points", "rt_closest_points_device", "rt_scene_closest_host"):
        assert name in abi.PROTOTYPES
        for lib in (rtlib, devlib):
            assert hasattr(lib, name), name
    assert [f[0] for f in abi.rt_point_query._fields_] == FIELDS
    assert rtlib.rt_abi_version() == 8 and "#define RT_ABI_VERSION 8" in header
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_mi355x.h"\nint main(void){printf("%zu\\n", sizeof(rt_point_query));' +
                   "".join(f'printf("%zu\\n", offsetof(rt_point_query, {f}));' for f in FIELDS) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", str(REPO / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(abi.rt_point_query)] + [getattr(abi.rt_point_query, f).offset for f in FIELDS]
    assert got[0] == 64


def _query(n=4, keep=None, **want):
    bufs = {"pos": np.zeros((4, 3), f32), "max_dist2": np.ones(4, f32), "dist2": np.zeros(4, f32), "u": np.zeros(4, f32), "v": np.zeros(4, f32),
            "tri": np.zeros(4, np.uint32), "point": np.zeros((4, 3), f32)}
    if keep is not None:
        keep.append(bufs)
    q = abi.rt_point_query(n=n)
    for name in FIELDS[1:]:
        setattr(q, name, bufs[name].ctypes.data if want.get(name, True) else None)
    return q


@pytest.mark.parametrize("entry", ["rt_closest_points", "rt_closest_points_device"])
def test_refusals_come_in_order_and_before_any_device_call(rtlib, entry):
    """On a host-only scene every status was decided in front of the device, in rt_trace_rays' order: RT_ERR_INVALID for a NULL scene or
    query; RT_OK for n == 0 whatever else is NULL; RT_ERR_INVALID for a NULL pos, then for every output NULL; RT_ERR_NO_DEVICE last."""
    s = Scene(scenes.get_scene("cornell"), device=-1)
    fn = getattr(rtlib, entry)
    call = (lambda h, q: fn(h, q)) if entry == "rt_closest_points" else (lambda h, q: fn(h, q, None))
    err = lambda: rtlib.rt_last_error().decode()
    keep = []
    inv = abi.RT_ERR_INVALID
    assert call(None, C.byref(_query(keep=keep))) == inv and "null argument" in err()
    assert call(s.h, None) == inv and "null argument" in err()
    none = {k: False for k in OUTPUTS}
    assert call(s.h, C.byref(_query(n=0, keep=keep))) == abi.RT_OK
    assert call(s.h, C.byref(_query(n=0, keep=keep, pos=False, **none))) == abi.RT_OK
    assert call(s.h, C.byref(_query(keep=keep, pos=False))) == inv and "pos" in err()
    assert call(s.h, C.byref(_query(keep=keep, pos=False, **none))) == inv and "pos" in err()  # pos before the outputs
    assert call(s.h, C.byref(_query(keep=keep, **none))) == inv and "output" in err()
    for kw in ({}, {"max_dist2": False}, {"dist2": False, "u": False, "v": False, "point": False}, {"tri": False}):
        assert call(s.h, C.byref(_query(keep=keep, **kw))) == abi.RT_ERR_NO_DEVICE, kw
        assert "host-only" in err()
    # what the host form refuses per entry comes after the device test: a host-only scene never gets that far
    bad = _query(keep=keep)
    keep[-1]["pos"][1, 0] = np.nan
    assert call(s.h, C.byref(bad)) == abi.RT_ERR_NO_DEVICE
    s.close()


def test_python_wrappers_refuse_wrong_shapes(rtlib):
    s = Scene(scenes.get_scene("cube"), device=-1)
    pos = np.zeros((2, 3), f32)
    with pytest.raises(abi.RtError) as e:
        s.closest_points(pos)
    assert e.value.status == abi.RT_ERR_NO_DEVICE
    for bad in ((np.zeros(6, f32), None), (np.zeros((2, 4), f32), None), (pos, np.ones(3, f32)), (pos, np.ones((2, 1), f32)), (pos, -1.0)):
        with pytest.raises(ValueError):
            s.closest_points(*bad)
    out = s.closest_points(np.zeros((0, 3), f32), 1.0)
    assert out["dist2"].shape == (0,) and out["point"].shape == (0, 3) and out["tri"].dtype == np.uint32 and out["dist"].shape == (0,)
    with pytest.raises(abi.RtError) as e:
        s.closest_points_device(5, 0, d_dist2=0)
    assert e.value.status == abi.RT_ERR_INVALID
    with pytest.raises(ValueError):
        s.closest_host(pos, max_dist2=np.ones(3, f32))
    assert rtlib.rt_scene_closest_host(s.h, 1, abi.fptr(pos), None, 2, None, None, None, None, None, None, None) == abi.RT_ERR_INVALID
    assert rtlib.rt_scene_closest_host(None, 0, None, None, 0, None, None, None, None, None, None, None) == abi.RT_ERR_INVALID
    assert rtlib.rt_scene_closest_host(s.h, 1, None, None, 0, None, None, None, None, None, None, None) == abi.RT_ERR_INVALID
    assert rtlib.rt_scene_closest_host(s.h, 2, abi.fptr(pos), None, 1, None, None, None, None, None, None, None) == abi.RT_OK  # every output NULL
    s.close()


def test_distance_grid_refuses_before_the_device_and_orders_points_as_a_probe_volume():
    s = Scene(scenes.get_scene("cube"), device=-1)
    for bad in (dict(origin=(0, 0), spacing=1.0, count=(1, 1, 1)), dict(origin=(0, 0, 0), spacing=(1.0, 2.0), count=(1, 1, 1)),
                dict(origin=(0, 0, 0), spacing=1.0, count=(1, 1)), dict(origin=(0, 0, 0), spacing=1.0, count=(1.5, 1, 1)),
                dict(origin=(0, 0, 0), spacing=1.0, count=(-1, 1, 1))):
        with pytest.raises(ValueError):
            bake.distance_grid(s, **bad)
    with pytest.raises(abi.RtError) as e:
        bake.distance_grid(s, (0, 0, 0), 0.5, (2, 3, 4))
    assert e.value.status == abi.RT_ERR_NO_DEVICE
    p = bake.grid_points((0.5, -1.0, 2.0), (0.1, 0.25, 0.5), (2, 3, 4))
    assert p.shape == (24, 3) and p.dtype == f32
    for (ix, iy, iz) in ((0, 0, 0), (1, 0, 0), (0, 2, 0), (1, 2, 3)):
        want = np.array([0.5, -1.0, 2.0], f32) + np.array([ix, iy, iz], f32) * np.array([0.1, 0.25, 0.5], f32)
        np.testing.assert_array_equal(p[(iz * 3 + iy) * 2 + ix], want)
    d, t = bake.distance_grid(s, (0, 0, 0), 0.5, (0, 3, 4))
    assert d.shape == (4, 3, 0) and t.shape == (4, 3, 0) and d.dtype == f32 and t.dtype == np.uint32
    s.close()


# ---- the contract: brute force against the model ----------------------------------------------------------------------------------------------
def _special_points(sd, wv):
    """every vertex, every edge's midpoint, every triangle's centre, the centre of the bounds"""
    lo, hi, _ = bounds_of(sd)
    w = wv.astype(np.float64)
    mids = 0.5 * (w + np.roll(w, 1, axis=1))
    return np.concatenate([w.reshape(-1, 3), mids.reshape(-1, 3), w.mean(1), [0.5 * (lo + hi)]]).astype(f32)


@pytest.mark.parametrize("name", ["triangle", "cube", "cornell"])
def test_host_brute_force_equals_the_model_bit_for_bit(rtlib, scene_cache, name):
    """rt_scene_closest_host(use_bvh = 0) == closest_model on 2,000 points: inside the bounds, outside on every side (near and 50 to 100
    scales out), on vertices, on edges, at triangle centres — and at the cube's centre, where twelve triangles tie and index 0 wins."""
    sd = scene_cache(name)
    wv = world_vertices(sd)
    special = _special_points(sd, wv)
    pos = np.concatenate([special, point_mix(sd, 2000 - len(special) % 2000, 11)])[:max(2000, len(special))]
    s = Scene(sd, device=-1)
    got = s.closest_host(pos)
    same(got, closest_model(pos, wv), name)
    assert (got["tri"] != NO_TRI).all() and np.isfinite(got["point"]).all()
    assert got["tri_tests"] == len(pos) * sd.n_triangles and got["node_visits"] == 0
    # with a radius of 1 % of the scale: misses appear, and they are the model's
    _, _, scale = bounds_of(sd)
    md2 = np.full(len(pos), f32(0.01 * scale) * f32(0.01 * scale), f32)
    got_r = s.closest_host(pos, max_dist2=md2)
    same(got_r, closest_model(pos, wv, md2), name + " radius")
    miss = got_r["tri"] == NO_TRI
    assert miss.any() and (~miss).any()
    assert np.isinf(got_r["dist2"][miss]).all() and np.isnan(got_r["point"][miss]).all() and (got_r["u"][miss] == 0).all() and (got_r["v"][miss] == 0).all()
    if name == "cube":
        lo, hi, _ = bounds_of(sd)
        c = (0.5 * (lo + hi)).astype(f32)[None]
        d2 = np.array([closest_candidates(c, w[0][None], (w[1] - w[0])[None], (w[2] - w[0])[None])[0][0] for w in wv])
        assert len(d2) == 12 and (d2 == d2[0]).all(), "the cube's twelve triangles tie at its centre"
        assert s.closest_host(c)["tri"][0] == 0
    s.close()


def test_vertices_of_the_scene_are_at_distance_zero(rtlib, scene_cache):
    sd = scene_cache("cornell")
    wv = world_vertices(sd)
    s = Scene(sd, device=-1)
    out = s.closest_host(wv.reshape(-1, 3))
    assert (out["dist2"] == 0).all()
    np.testing.assert_array_equal(out["point"], wv.reshape(-1, 3))
    assert (out["tri"] <= np.repeat(np.arange(sd.n_triangles), 3)).all()  # the lowest index among the triangles that share the vertex
    s.close()


def test_a_zero_area_triangle_never_wins_where_its_dist2_is_nan(rtlib):
    """Triangle 0 has v1 == v0 (e1 = 0: the segment v0 v2), triangle 1 is a segment with e2 = 2 e1, triangle 2 a point, triangle 3 a proper
    one. For triangle 0 and a point with e2 . ap > 0 the walk reaches the edge region of e1 with d1 = d3 = 0: u = 0 / 0, dist2 is NaN. Such
    a candidate never counts, and the winner is the model's; walks and brute force agree."""
    tris = [[[0, 0, 1], [0, 0, 1], [0, 0, 2]], [[2, 0, 0], [3, 0, 0], [4, 0, 0]], [[1, 1, 1]] * 3, [[0, 0, 0], [1, 0, 0], [0, 1, 0]]]
    sd = tri_scene("degenerate", tris)
    wv = world_vertices(sd)
    g = np.random.default_rng(4)
    pos = np.concatenate([g.uniform(-2, 5, (1500, 3)), [[0, 0, 1], [0.2, 0.2, 3.0], [2.5, 0, 0], [3.5, 1, 0]]]).astype(f32)
    d2 = closest_candidates(pos, wv[0, 0][None], (wv[0, 1] - wv[0, 0])[None], (wv[0, 2] - wv[0, 0])[None])[0]
    assert np.isnan(d2).mean() > 0.3 and not np.isnan(d2).all(), "the e1 = 0 triangle gives NaN above its first vertex"
    want = closest_model(pos, wv)
    assert (want["tri"][np.isnan(d2)] != 0).all() and (want["tri"] != NO_TRI).all() and not np.isnan(want["dist2"]).any()
    for bvh in (abi.RT_BVH_SAH, abi.RT_BVH_LBVH):
        s = Scene(sd, device=-1, bvh=bvh)
        same(s.closest_host(pos), want, "brute")
        same(s.closest_host(pos, use_bvh=True), want, "walk")
        s.close()
    only = tri_scene("segment", tris[:1])  # alone: a miss wherever its dist2 is NaN
    s = Scene(only, device=-1)
    got = s.closest_host(pos)
    same(got, closest_model(pos, world_vertices(only)), "point alone")
    assert ((got["tri"] == NO_TRI) == np.isnan(d2)).all()
    s.close()


def test_a_radius_on_the_winners_dist2_counts_and_the_next_float_below_misses(rtlib, scene_cache):
    sd = scene_cache("cornell")
    wv = world_vertices(sd)
    pos = point_mix(sd, 1200, 8, far=0.1)
    s = Scene(sd, device=-1)
    free = s.closest_host(pos)
    d2 = free["dist2"]
    for use_bvh in (False, True):
        same(s.closest_host(pos, max_dist2=d2, use_bvh=use_bvh), free, "radius == dist2")
        below = np.nextafter(d2, f32(-np.inf))
        got = s.closest_host(pos, max_dist2=below, use_bvh=use_bvh)
        same(got, closest_model(pos, wv, below), "radius just below")
        assert (got["tri"] == NO_TRI).all() and np.isinf(got["dist2"]).all()
        inf = s.closest_host(pos, max_dist2=np.full(len(pos), np.inf, f32), use_bvh=use_bvh)
        same(inf, free, "radius +inf")
        neg = s.closest_host(pos, max_dist2=np.full(len(pos), -1.0, f32), use_bvh=use_bvh)
        assert (neg["tri"] == NO_TRI).all()
        # -0.0 admits dist2 == 0 (0 <= -0.0) and nothing else: the scene's vertices hit, the mix's other points miss
        v = wv.reshape(-1, 3)[:200]
        mz = s.closest_host(np.concatenate([v, pos]), max_dist2=np.full(len(v) + len(pos), -0.0, f32), use_bvh=use_bvh)
        assert (mz["tri"][:len(v)] != NO_TRI).all() and (mz["dist2"][:len(v)] == 0).all()
        assert ((mz["tri"][len(v):] == NO_TRI) == (d2 != 0)).all()
        nan = s.closest_host(pos[:50], max_dist2=np.full(50, np.nan, f32), use_bvh=use_bvh)  # (the diagnostic refuses nothing: a miss)
        assert (nan["tri"] == NO_TRI).all()
    s.close()


def _true_distance(p, a, b, c):
    """float64 distance from points p (n, 3) to triangles (a, b, c) (n, 3) each: the minimum over the plane patch's interior projection
    (where inside) and the three edges' segments — no region logic shared with the model."""
    def seg(p, a, b):
        ab = b - a
        den = (ab * ab).sum(1)
        t = np.clip(((p - a) * ab).sum(1) / np.where(den > 0, den, 1.0), 0.0, 1.0)
        return np.linalg.norm(p - (a + t[:, None] * ab), axis=1)
    d = np.minimum(np.minimum(seg(p, a, b), seg(p, b, c)), seg(p, c, a))
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(1)
    ok = nn > 0
    nn = np.where(ok, nn, 1.0)
    h = ((p - a) * n).sum(1) / nn
    q = p - h[:, None] * n
    inside = ok
    for x, y in ((a, b), (b, c), (c, a)):
        inside = inside & ((np.cross(y - x, q - x) * n).sum(1) >= 0)
    return np.where(inside, np.minimum(d, np.abs(h) * np.sqrt(nn)), d)


@pytest.mark.parametrize("scales", [1.0, 100.0])
def test_the_model_never_underestimates_the_true_distance_by_more_than_the_bound(scales):
    """sqrt(dist2) >= d_true - 8 * 2^-24 * (|ap| + |e1| + |e2|) against a float64 restatement, on 200,000 random pairs: well-shaped
    triangles, slivers with |e1||e2| / |e1 x e2| up to ~10^5, and points `scales` triangle sizes away. The cull leans on this side alone."""
    g = np.random.default_rng(int(scales))
    n = 200_000
    v0 = g.uniform(-1, 1, (n, 3))
    e1 = g.normal(size=(n, 3)) * 10.0 ** g.uniform(-2, 0, (n, 1))
    e2 = g.normal(size=(n, 3)) * 10.0 ** g.uniform(-2, 0, (n, 1))
    sliver = np.arange(n) % 3 == 0
    e2 = np.where(sliver[:, None], e1 * g.uniform(-2, 2, (n, 1)) + e2 * 10.0 ** g.uniform(-5, -2, (n, 1)), e2)
    p = v0 + g.normal(size=(n, 3)) * scales * 10.0 ** g.uniform(-2, 0, (n, 1))
    p, v0, e1, e2 = (x.astype(f32) for x in (p, v0, e1, e2))
    d2, u, v, r = closest_candidates(p, v0, e1, e2)
    ok = ~np.isnan(d2)
    assert ok.mean() > 0.999
    P, A, E1, E2 = (x.astype(np.float64) for x in (p, v0, e1, e2))
    true = _true_distance(P, A, A + E1, A + E2)
    unit = 2.0 ** -24 * (np.linalg.norm(P - A, axis=1) + np.linalg.norm(E1, axis=1) + np.linalg.norm(E2, axis=1))
    short = (true - np.sqrt(d2.astype(np.float64))) / unit
    print(f"underestimate at {scales} scales: worst {short[ok].max():.2f} units of 2^-24 (|ap| + |e1| + |e2|) (bound 8)")
    assert short[ok].max() <= 8.0


# ---- the walk: the tree only culls ----------------------------------------------------------------------------------------------------------
def _walk_cases():
    from test_scene_update import chain_scene, update_sequence
    def updated(lib):
        sd = scenes.get_scene("atrium", detail=1)
        s = Scene(sd, -1, abi.RT_BVH_LBVH, lib=lib, updatable=True)
        for u in update_sequence(sd)[:2]:
            s.update(**u)
        return s
    return {
        "sah_presplit": lambda lib: Scene(scenes.atrium_tilted_scene(1), -1, abi.RT_BVH_SAH, lib=lib),
        "median": lambda lib: Scene(chain_scene(), -1, abi.RT_BVH_LBVH, lib=lib),
        "updated": updated,
        "atrium_sah": lambda lib: Scene(scenes.get_scene("atrium", detail=1), -1, abi.RT_BVH_SAH, lib=lib),
        "atrium_lbvh": lambda lib: Scene(scenes.get_scene("atrium", detail=1), -1, abi.RT_BVH_LBVH, lib=lib),
        "rotated_lbvh": lambda lib: Scene(scenes.atrium_tilted_scene(1), -1, abi.RT_BVH_LBVH, lib=lib),
        "tables": lambda lib: Scene(scenes.table_scene(), -1, abi.RT_BVH_SAH, lib=lib),
        "empty": lambda lib: Scene(scenes.get_scene("empty"), -1, abi.RT_BVH_SAH, lib=lib),
    }


@pytest.mark.parametrize("case", ["sah_presplit", "median", "updated", "atrium_sah", "atrium_lbvh", "rotated_lbvh", "tables", "empty"])
def test_the_walk_equals_the_brute_force_on_every_builder(devlib, case):
    """rt_scene_closest_host: use_bvh = 1 (the kernel's cull rule and child order on the decoded boxes) == use_bvh = 0 bit for bit on
    20,000 points, a third of them 50 to 100 scene scales outside, with no radius and with one of 1 % of the scale, on every builder a
    host-only scene can have: SAH with pre-split triangles, the median fallback, an updatable scene after updates, SAH and LBVH on the atrium
    at detail 1 and on its rotated copy, the table scene, the empty scene. The walk visits far fewer nodes than points x nodes."""
    s = _walk_cases()[case](devlib)
    info, tree = s.info(), s.tree()
    if case == "sah_presplit":
        assert info.n_split_triangles > 0
    if case == "median":
        assert tree["built_by"] == abi.RT_BVH_MEDIAN_INTERNAL
    s.check_bvh()
    sd = s.desc
    n = 20_000
    pos = point_mix(sd, n, 21)
    _, _, scale = bounds_of(sd)
    for radius in (None, f32(0.01 * scale)):
        md2 = None if radius is None else np.full(n, radius * radius, f32)
        brute, walk = s.closest_host(pos, md2), s.closest_host(pos, md2, use_bvh=True)
        same(walk, brute, f"{case} radius {radius}")
        if case == "empty":
            assert (walk["tri"] == NO_TRI).all() and walk["tri_tests"] == 0 and walk["node_visits"] == n
            continue
        assert brute["tri_tests"] == n * info.n_leaf_records
        per_point = walk["node_visits"] / n
        print(f"{case} radius {radius}: {per_point:.1f} node visits and {walk['tri_tests'] / n:.1f} triangle tests per point "
              f"({info.n_nodes} nodes, {info.n_leaf_records} records)")
        # "far below": a tenth, on trees of a thousand nodes or more. A walk visits a node per level at the least, which on the chain
        # scene (23 nodes over 40 copies of each triangle, equal candidates the tie rule makes it visit) and the table scene (61 nodes)
        # is already more than a tenth of the tree: there the walk has to stay under the whole tree.
        share = 0.1 if info.n_nodes >= 1000 else 1.0
        assert (info.n_nodes >= 1000) == (case not in ("median", "tables"))
        assert walk["node_visits"] < share * n * info.n_nodes and walk["tri_tests"] < share * brute["tri_tests"]
        if radius is None:
            assert (walk["tri"] != NO_TRI).all()
        else:
            hit = walk["tri"] != NO_TRI
            assert hit.any() and (~hit).any() and (walk["dist2"][hit] <= md2[hit]).all()
    s.close()


def test_the_walk_after_an_update_equals_a_fresh_build(devlib):
    from test_scene_update import update_sequence
    sd = scenes.get_scene("atrium", detail=1)
    s = Scene(sd, -1, abi.RT_BVH_SAH, lib=devlib, updatable=True)
    s.update(**update_sequence(sd)[0])
    fresh = Scene(s.desc, -1, abi.RT_BVH_SAH, lib=devlib)
    pos = point_mix(s.desc, 4000, 3)
    same(s.closest_host(pos, use_bvh=True), fresh.closest_host(pos, use_bvh=True), "updated vs fresh")
    s.close(), fresh.close()


# ---- the listing --------------------------------------------------------------------------------------------------------------------------
K_CLOSEST = "_ZN2rt9k_closestENS_8SceneDevENS_8PointDevE"


def test_closest_kernel_has_the_resources_design_states_and_no_scratch_beyond_the_spill_array(tmp_path):
    """k_closest (rt_closest.hip): registers, spills, scratch, LDS and occupancy are the figures of DESIGN.md §22, read from the listing and
    from DESIGN.md itself. The scratch is the traversal stack's spill array (52 words, rounded up to 16 bytes) and nothing else: no
    register is spilled. The node fetch is plain loads, so the ISA hazard scan of the asm-issued fetch has nothing to look at here."""
    from test_denoise import _listing
    from test_svgf import _metadata
    lines = _listing("rt_closest.hip", tmp_path)
    meta = "\n".join(lines)
    got = {k: _metadata(meta, K_CLOSEST, k) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                                                       "group_segment_fixed_size")}
    occ = [int(m) for m in re.findall(r"^; Occupancy: (\d+)", meta, re.M)]
    assert len(occ) == 1  # one kernel in the unit
    got["occupancy"] = occ[0]
    design = (REPO / "DESIGN.md").read_text()
    m = re.search(r"`k_closest`: (\d+) VGPRs, (\d+) spilled, (\d+) bytes of scratch per lane, ([\d,]+) bytes of LDS per workgroup, (\d+) waves per SIMD", design)
    assert m, "DESIGN.md states k_closest's resources in one sentence"
    stated = {"vgpr_count": int(m.group(1)), "vgpr_spill_count": int(m.group(2)), "sgpr_spill_count": 0, "private_segment_fixed_size": int(m.group(3)),
              "group_segment_fixed_size": int(m.group(4).replace(",", "")), "occupancy": int(m.group(5))}
    assert got == stated
    # the frame is the spill array's 52 words and the padding hipcc gives every kernel with RT_TRAVERSAL_LDS's array (k_query's frame); the only
    # scratch instructions are that array's, addressed by the entry's register, never a spill slot's constant offset
    kq = _metadata("\n".join(_listing("rt_query.hip", tmp_path)), "_ZN2rt7k_queryILb0EEEvNS_8SceneDevENS_8QueryDevE", "private_segment_fixed_size")
    assert got["vgpr_spill_count"] == 0 and 4 * (64 - 12) <= got["private_segment_fixed_size"] == kq
    scratch = [ln.strip() for ln in lines if re.match(r"\s+scratch_", ln)]
    assert 1 <= len(scratch) <= 8 and all(re.fullmatch(r"scratch_(load|store)_dword v\d+, v\d+, off", ln) for ln in scratch), scratch
    assert got["occupancy"] == 6 and got["vgpr_count"] <= 80 and 3 * got["group_segment_fixed_size"] <= 160 * 1024
    assert "global_load_dwordx4 %" not in (REPO / "sycl-ray-tracer_amd" / "csrc" / "rt_closest.hip").read_text()


# ---- the trees the kernel's own steps are held on (tests/test_gpu_closest_points_trees.py): their host statement ----------------------------
# tests/closest_scenes.py imports this module, so it is imported inside the functions here.
TREE_CASES = ["pile", "offset_near", "offset_far", "mixed", "mixed_corner", "duplicates"]
_tree_cache = {}


def _tree_case(case):
    """-> dict(sd, pos, wv, mask, model): the scene, its 4,096 points (the pile: 1,024 more in its free corner; the offset atria: 2,048), and on the mixed and the
    duplicate scenes closest_model without a radius. Built once per case and shared by the builders; nothing changes it."""
    import closest_scenes as cs
    if case in _tree_cache:
        return _tree_cache[case]
    mask = None
    if case == "pile":
        sd = cs.pile_scene()
        pos = np.concatenate([point_mix(sd, 4096, 1), cs.pile_corner_points(1024, 2)])
    elif case in ("offset_near", "offset_far"):
        sd = cs.offset_scene(cs.OFFSETS[case == "offset_far"])
        pos = point_mix(sd, 2048, 2)  # (18,604 records: the brute force is the cost)
    elif case in ("mixed", "mixed_corner"):
        sd, mask = cs.mixed_scene()
        pos = point_mix(sd, 4096, 7) if case == "mixed" else cs.corner_points(sd, 4096, 3)
    else:
        sd = cs.duplicate_scene()
        pos = point_mix(sd, 4096, 4)
    wv = world_vertices(sd)
    np.testing.assert_array_equal(wv, sd.world_triangles().astype(f32).reshape(-1, 3, 3))  # tri_scene: world vertices = positions
    model = closest_model(pos, wv) if case in ("mixed", "mixed_corner", "duplicates") else None
    _tree_cache[case] = dict(sd=sd, pos=pos, wv=wv, mask=mask, model=model)
    return _tree_cache[case]


@pytest.mark.parametrize("builder", ["sah", "lbvh"])
@pytest.mark.parametrize("case", TREE_CASES)
def test_the_walk_equals_the_brute_force_on_the_trees_the_device_is_held_on(devlib, case, builder):
    """On the pile (stack_need > 12 under both builders), the atrium moved to (1000, -2000, 500) and to (1e5, 1e5, 1e5), the mixed scene
    with its 300 degenerate triangles (pre-split under SAH) at the point mix and in the corner of the contract range, and seven shuffled
    copies of the cube: check_bvh passes, the walk equals the brute force bit for bit with no radius and with radius_mix, and on the mixed
    and duplicate scenes the brute force equals closest_model. On the duplicates every winner is the lowest copy of its triangle."""
    import closest_scenes as cs
    c = _tree_case(case)
    sd, pos = c["sd"], c["pos"]
    s = Scene(sd, -1, cs.BUILDERS[builder], lib=devlib)
    s.check_bvh()
    info, tree = s.info(), s.tree()
    assert tree["built_by"] == cs.BUILDERS[builder]
    if case == "pile":
        assert tree["stack_need"] > cs.K_LDS_STACK
    if case in ("mixed", "mixed_corner"):
        assert (info.n_split_triangles > 0) == (builder == "sah")
    brute, walk = s.closest_host(pos), s.closest_host(pos, use_bvh=True)
    same(walk, brute, f"{case} {builder}")
    assert (brute["tri"] != NO_TRI).all() and not np.isnan(brute["dist2"]).any()
    print(f"{case} {builder}: {info.n_nodes} nodes, {info.n_leaf_records} records, depth {info.max_depth}, stack_need {tree['stack_need']}, "
          f"{info.n_split_triangles} pre-split; the walk: {walk['node_visits'] / len(pos):.1f} node visits and {walk['tri_tests'] / len(pos):.1f} "
          f"triangle tests per point with no radius")
    md2 = cs.radius_mix(brute["dist2"], 5)
    brute_r = s.closest_host(pos, md2)
    same(s.closest_host(pos, md2, use_bvh=True), brute_r, f"{case} {builder}, radius_mix")
    hit = brute_r["tri"] != NO_TRI
    assert hit.any() and (~hit).any()
    if c["model"] is not None:
        same(brute, c["model"], f"{case} {builder}: brute force vs model")
        if builder == "sah":  # (the model takes seconds on the mixed scene: with radii once per case, on the first 1,024 entries)
            same({k: brute_r[k][:1024] for k in OUTPUTS}, closest_model(pos[:1024], c["wv"], md2[:1024]), f"{case}: brute force vs model, radius_mix")
    if case == "duplicates":
        np.testing.assert_array_equal(brute["tri"], cs.lowest_copy(brute["tri"]))
        np.testing.assert_array_equal(brute_r["tri"][hit], cs.lowest_copy(brute_r["tri"][hit]))
        assert len(np.unique(brute["tri"])) == 12
    s.close()


def test_the_mixed_scene_gives_nan_candidates_and_degenerate_winners():
    """What the mixed scene is there for, stated on the model: every degenerate triangle of kind (a, a, b) gives a NaN candidate for some
    of the 4,096 points, no winner is NaN, and some winners are degenerate triangles (the regions where their dist2 is finite)."""
    import closest_scenes as cs
    c = _tree_case("mixed")
    wv, mask, pos, model = c["wv"], c["mask"], c["pos"], c["model"]
    assert mask.sum() == 300 and len(wv) == 3802
    src = cs.nan_source(wv, mask)
    assert len(src) == 100
    d2 = closest_candidates(pos[:, None], wv[src, 0][None], (wv[src, 1] - wv[src, 0])[None], (wv[src, 2] - wv[src, 0])[None])[0]
    nans = np.isnan(d2).sum(0)
    print(f"{nans.sum()} NaN candidates over {len(src)} triangles x {len(pos)} points, at least {nans.min()} per triangle; "
          f"{mask[model['tri']].sum()} degenerate winners")
    assert (nans >= 1).all()
    assert not np.isnan(model["dist2"]).any() and (model["tri"] != NO_TRI).all()
    assert mask[model["tri"]].sum() >= 1
    # without the degenerate triangles the same seed gives the same other triangles: the degenerate ones are an addition
    plain, none = cs.mixed_vertices(degenerate=False)
    assert not none.any() and len(plain) == 3502
    assert {t.tobytes() for t in plain} == {t.tobytes() for t in wv[~mask]}


def test_vertex_radii_hit_at_zero_and_miss_below_it(devlib):
    """The first 1,000 world vertices of the Cornell box and of the mixed scene as points, with max_dist2 cycling through -0.0, +0.0,
    FLT_MIN and +inf (hits with dist2 == 0 and the vertex as point) and -1 (a miss): brute force, walk and model. On the mixed scene a
    third vertex need not be at 0 (closest_scenes.check_vertex_radii says why): there the model alone is the statement."""
    import closest_scenes as cs
    for name, sd in (("cornell", scenes.get_scene("cornell")), ("mixed", _tree_case("mixed")["sd"])):
        wv = world_vertices(sd)
        n = min(1000, 3 * len(wv) // 5 * 5)
        pos, md2 = cs.vertex_radii(wv, n)
        want = closest_model(pos, wv, md2)
        cs.check_vertex_radii(want, pos, md2, name, third_vertices=name == "cornell")
        for builder in ("sah", "lbvh"):
            s = Scene(sd, -1, cs.BUILDERS[builder], lib=devlib)
            same(s.closest_host(pos, md2), want, f"{name} {builder} brute")
            same(s.closest_host(pos, md2, use_bvh=True), want, f"{name} {builder} walk")
            s.close()
