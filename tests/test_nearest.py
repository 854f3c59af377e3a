"""k-nearest closest-point queries (include/rt_mi355x.h: rt_closest_points_multi[_device], rt_scene_nearest_host) without a GPU: the
exported entry points and the struct layout, the refusals in front of the device, the Python wrappers, the host brute force and the host
walk against the numpy model (tests/nearest_scenes.py) on the three small scenes — free, under radii and with keys —, the k = 1, paging,
exhaustion and range identities, radius and key edges, the walk (the kernel's moving bound and de-duplication) against the brute force on
every builder and on the harder trees, what the bound saves, contact_points, what the kernel leans on in the point traversal, and the
kernels' listing: resources as DESIGN.md §25 states them. Every comparison is bit for bit."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import closest_scenes as cs
import nearest_scenes as ns
from nearest_scenes import SLOTS, key_mix, nearest_model, paged, same, small_case
from rtamd import abi, bake, scenes
from rtamd.renderer import Scene
from test_closest_points import NO_TRI, bounds_of, closest_model, point_mix, world_vertices

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "sycl-ray-tracer_amd" / "csrc"
f32 = np.float32
FIELDS = ["n", "k", "pos", "max_dist2", "after_dist2", "after_tri", "dist2", "u", "v", "tri", "count"]
SMALL = ["cornell", "duplicates", "pile256"]


# ---- the surface --------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_prototyped(rtlib, devlib, tmp_path):
    header = (REPO / "include" / "rt_mi355x.h").read_text()
    assert "typedef struct rt_nearest_query {" in header and "#define RT_NEAREST_MAX 8" in header and abi.RT_NEAREST_MAX == 8
    for name in ("rt_closest_points_multi", "rt_closest_points_multi_device"):
        assert re.search(rf"^int {name}\(rt_scene\* scene, const rt_nearest_query\* q", header, re.M), name
    assert re.search(r"^int rt_scene_nearest_host\(const rt_scene\* scene, uint32_t n, uint32_t k, const float\* pos, const float\* max_dist2, "
                     r"const float\* after_dist2,\s+const uint32_t\* after_tri, int use_bvh, float\* dist2, float\* u, float\* v, uint32_t\* tri, "
                     r"uint32_t\* count,\s+uint64_t\* node_visits, uint64_t\* tri_tests\);", header, re.M)
    for name in ("rt_closest_points_multi", "rt_closest_points_multi_device", "rt_scene_nearest_host"):
        assert name in abi.PROTOTYPES
        for lib in (rtlib, devlib):
            assert hasattr(lib, name), name
    assert [f[0] for f in abi.rt_nearest_query._fields_] == FIELDS
    assert rtlib.rt_abi_version() == 8 and "#define RT_ABI_VERSION 8" in header
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_mi355x.h"\nint main(void){printf("%zu\\n", sizeof(rt_nearest_query));' +
                   "".join(f'printf("%zu\\n", offsetof(rt_nearest_query, {f}));' for f in FIELDS) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", str(REPO / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(abi.rt_nearest_query)] + [getattr(abi.rt_nearest_query, f).offset for f in FIELDS]
    assert got[0] == 80
    internal = (CSRC / "rt_internal.h").read_text()
    assert "kQueryKindNearest = 8, kQueryKinds = 11" in internal


def _query(n=4, k=2, keep=None, **want):
    bufs = {"pos": np.zeros((4, 3), f32), "max_dist2": np.ones(4, f32), "after_dist2": np.zeros(4, f32), "after_tri": np.zeros(4, np.uint32),
            "dist2": np.zeros((4, 8), f32), "u": np.zeros((4, 8), f32), "v": np.zeros((4, 8), f32), "tri": np.zeros((4, 8), np.uint32),
            "count": np.zeros(4, np.uint32)}
    if keep is not None:
        keep.append(bufs)
    q = abi.rt_nearest_query(n=n, k=k)
    for name in FIELDS[2:]:
        setattr(q, name, bufs[name].ctypes.data if want.get(name, True) else None)
    return q


@pytest.mark.parametrize("entry", ["rt_closest_points_multi", "rt_closest_points_multi_device"])
def test_refusals_come_in_order_and_before_any_device_call(rtlib, entry):
    """On a host-only scene every status was decided in front of the device, in query_check's order: RT_ERR_INVALID for a NULL scene or
    query; RT_OK for n == 0 whatever else is wrong; RT_ERR_INVALID for k outside 1 .. 8, then a NULL pos, then half a key, then every
    output NULL; RT_ERR_NO_DEVICE last."""
    s = Scene(scenes.get_scene("cornell"), device=-1)
    fn = getattr(rtlib, entry)
    call = (lambda h, q: fn(h, q)) if entry == "rt_closest_points_multi" else (lambda h, q: fn(h, q, None))
    err = lambda: rtlib.rt_last_error().decode()
    keep = []
    inv = abi.RT_ERR_INVALID
    none = {k: False for k in ns.OUTPUTS}
    assert call(None, C.byref(_query(keep=keep))) == inv and "null argument" in err()
    assert call(s.h, None) == inv and "null argument" in err()
    assert call(s.h, C.byref(_query(n=0, keep=keep))) == abi.RT_OK
    assert call(s.h, C.byref(_query(n=0, k=0, keep=keep, pos=False, after_dist2=False, **none))) == abi.RT_OK
    for k in (0, 9, 0xFFFFFFFF):
        assert call(s.h, C.byref(_query(k=k, keep=keep))) == inv and "k must be" in err()
        assert call(s.h, C.byref(_query(k=k, keep=keep, pos=False, after_tri=False, **none))) == inv and "k must be" in err()  # k first
    assert call(s.h, C.byref(_query(keep=keep, pos=False))) == inv and "pos" in err()
    assert call(s.h, C.byref(_query(keep=keep, pos=False, after_dist2=False, **none))) == inv and "pos" in err()  # before the key
    for kw in ({"after_dist2": False}, {"after_tri": False}):
        assert call(s.h, C.byref(_query(keep=keep, **kw))) == inv and "key" in err()
        assert call(s.h, C.byref(_query(keep=keep, **kw, **none))) == inv and "key" in err()  # the key before the outputs
    assert call(s.h, C.byref(_query(keep=keep, **none))) == inv and "output" in err()
    for kw in ({}, {"max_dist2": False}, {"after_dist2": False, "after_tri": False}, {"dist2": False, "u": False, "v": False, "tri": False},
               {"count": False}, {"k": 1}, {"k": 8}):
        assert call(s.h, C.byref(_query(keep=keep, **kw))) == abi.RT_ERR_NO_DEVICE, kw
        assert "host-only" in err()
    # what the host form refuses per entry comes after the device test: a host-only scene never gets that far
    bad = _query(keep=keep)
    keep[-1]["after_dist2"][1] = np.nan
    assert call(s.h, C.byref(bad)) == abi.RT_ERR_NO_DEVICE
    s.close()


def test_python_wrappers_refuse_wrong_shapes_and_dtypes(rtlib):
    s = Scene(scenes.get_scene("cube"), device=-1)
    pos = np.zeros((2, 3), f32)
    with pytest.raises(abi.RtError) as e:
        s.closest_points_multi(pos, 2)
    assert e.value.status == abi.RT_ERR_NO_DEVICE
    key = (np.zeros(2, f32), np.zeros(2, np.uint32))
    bad = [dict(pos=np.zeros(6, f32)), dict(pos=np.zeros((2, 4), f32)), dict(k=0), dict(k=9), dict(k=2.0), dict(k=True),
           dict(max_dist=np.ones(3, f32)), dict(max_dist=np.ones((2, 1), f32)), dict(max_dist=np.array(["a", "b"])), dict(max_dist=-1.0),
           dict(after=key[0]), dict(after=(key[0],)), dict(after=(key[0], np.zeros(2, f32))), dict(after=(np.zeros(2, np.int32), key[1])),
           dict(after=(np.zeros(3, f32), np.zeros(3, np.uint32)))]
    for kw in bad:
        args = dict(pos=pos, k=2)
        args.update(kw)
        with pytest.raises(ValueError):
            s.closest_points_multi(**args)
        if kw.get("k") != 9 and "max_dist" not in kw:  # (the host diagnostic takes any k >= 1, and squared radii of any value)
            with pytest.raises(ValueError):
                s.nearest_host(**args)
    with pytest.raises(ValueError):
        s.nearest_host(pos, 2, max_dist2=np.ones(3, f32))
    for kw in (dict(max_dist=1.0, page=0), dict(max_dist=1.0, page=9), dict(max_dist=1.0, max_items=0), dict(max_dist=1.0, max_items=1.5),
               dict(max_dist=np.ones(3, f32)), dict(max_dist=-1.0), dict(max_dist=None)):
        with pytest.raises(ValueError):
            s.closest_all(pos, **kw)
    off = s.closest_all(pos, None, max_items=3)[0]  # no radius is taken with a bound on the items
    np.testing.assert_array_equal(np.diff(off), [3, 3])
    out = s.nearest_host(np.zeros((0, 3), f32), 3)
    assert out["dist2"].shape == (0, 3) and out["tri"].dtype == np.uint32 and out["count"].shape == (0,)
    with pytest.raises(abi.RtError) as e:
        s.closest_points_multi_device(5, 2, 0)
    assert e.value.status == abi.RT_ERR_INVALID
    with pytest.raises(ValueError):
        bake.triangles_within(s, pos, None)
    with pytest.raises(ValueError):
        bake.triangles_within(s, np.zeros((2, 2), f32), 1.0)
    wv = world_vertices(s.desc)
    z, zi = np.zeros(2, f32), np.zeros(2, np.uint32)
    for args in ((wv[:, :2], pos, z, z, zi), (wv, np.zeros((2, 2), f32), z, z, zi), (wv, pos, z, z[:1], zi), (wv, pos, z, z, z),
                 (wv, pos, z, z, np.full(2, 12, np.uint32)), (wv, pos, np.zeros((2, 2, 2), f32), np.zeros((2, 2, 2), f32), np.zeros((2, 2, 2), np.uint32))):
        with pytest.raises(ValueError):
            bake.contact_points(*args)
    host = rtlib.rt_scene_nearest_host
    p = abi.fptr(pos)
    assert host(None, 0, 1, None, None, None, None, 0, None, None, None, None, None, None, None) == abi.RT_ERR_INVALID
    assert host(s.h, 1, 1, None, None, None, None, 0, None, None, None, None, None, None, None) == abi.RT_ERR_INVALID
    assert host(s.h, 1, 1, p, None, None, None, 2, None, None, None, None, None, None, None) == abi.RT_ERR_INVALID
    assert host(s.h, 1, 0, p, None, None, None, 0, None, None, None, None, None, None, None) == abi.RT_ERR_INVALID
    assert host(s.h, 1, 1, p, None, abi.fptr(key[0]), None, 0, None, None, None, None, None, None, None) == abi.RT_ERR_INVALID
    assert host(s.h, 2, 40, p, None, None, None, 1, None, None, None, None, None, None, None) == abi.RT_OK  # every output NULL, k > 8
    s.close()


# ---- the three small scenes against the model ----------------------------------------------------------------------------------------------
def test_the_small_scenes_meet_the_conditions_their_tests_lean_on():
    """Cornell: at least 30 % of the points have 9 or more triangles within 0.25 scene scales. The duplicates: for every k in 1 .. 8 a tie
    straddles slot k - 1 on every point, without a key or behind the first entry's key. The pile of 256: every point fills 8 slots."""
    c = small_case("cornell")
    n = len(c["pos"])
    w = ns.within(c["table"], ns.squared_radius(c["scale"], 0.25, n))
    none = ns.within(c["table"], ns.squared_radius(c["scale"], 0.1, n)) == 0
    m2 = nearest_model(c["table"], 2)
    print(f"cornell: {100.0 * (w >= 9).mean():.1f} % of the points have >= 9 triangles within 0.25 scales, at most {w.max()}; "
          f"{100.0 * none.mean():.1f} % have none within 0.1; {100.0 * (m2['dist2'][:, 0] == m2['dist2'][:, 1]).mean():.1f} % tie on the first two")
    assert (w >= 9).mean() >= 0.30
    dup = small_case("duplicates")["table"]
    for k in range(1, 9):
        free, keyed = ns.tie_straddles(dup, k), ns.tie_straddles(dup, k, ns.first_key(dup))
        print(f"duplicates k={k}: a tie straddles slot k - 1 on {100.0 * free.mean():.1f} % of the points without a key, {100.0 * keyed.mean():.1f} % behind the first entry's")
        assert (free | keyed).all(), k
    p = small_case("pile256")["table"]
    m9 = nearest_model(p, 9)
    print(f"pile256: at least {np.isfinite(p['dist2']).sum(0).min()} finite candidates per point, {100.0 * (np.diff(m9['dist2'], axis=1) == 0).any(1).mean():.1f} % tie among the first 9")
    assert (nearest_model(p, 8)["count"] == 8).all() and (m9["count"] == 9).all()


@pytest.fixture(scope="module")
def host_scenes(rtlib):
    made = {name: Scene(small_case(name)["sd"], device=-1) for name in SMALL}
    yield made
    for s in made.values():
        s.close()


@pytest.mark.parametrize("name", SMALL)
def test_the_brute_force_and_the_walk_equal_the_model(host_scenes, name):
    """nearest_host(use_bvh = 0) == nearest_host(use_bvh = 1) == nearest_model for k = 1, 2, 3 and 8: free, under radius_mix around the
    first entry and around the k-th, and with the keys of the key mix; on the duplicates also behind every point's first entry."""
    c, s = small_case(name), host_scenes[name]
    pos, tab = c["pos"], c["table"]
    free8 = nearest_model(tab, 8)
    md_mix, after = key_mix(free8, 3)
    for k in (1, 2, 3, 8):
        runs = [("free", None, None), ("radius_mix on the first", cs.radius_mix(free8["dist2"][:, 0], 5), None),
                ("radius_mix on the k-th", cs.radius_mix(free8["dist2"][:, k - 1], 6), None), ("keys", None, after), ("radii and keys", md_mix, after)]
        if name == "duplicates":
            runs += [(what, None, key) for what, key in ns.duplicate_runs(tab, k)[1:]]
        for what, md2, key in runs:
            want = nearest_model(tab, k, md2, key)
            same(s.nearest_host(pos, k, md2, key), want, f"{name} k={k} {what}: brute force")
            same(s.nearest_host(pos, k, md2, key, use_bvh=True), want, f"{name} k={k} {what}: walk")
            filled = np.arange(k)[None, :] < want["count"][:, None]
            assert ((want["tri"] != NO_TRI) == filled).all() and np.isinf(want["dist2"][~filled]).all()
            assert (want["u"][~filled] == 0).all() and (want["v"][~filled] == 0).all()
            if md2 is not None:
                assert (want["count"] < k).any() and (want["count"] > 0).any(), (name, k, what)


@pytest.mark.parametrize("name", SMALL)
def test_k_1_is_the_closest_point(host_scenes, name):
    """With k = 1 and no key the slot is closest_model's and rt_scene_closest_host's dist2, u, v, tri bit for bit, free and under radii."""
    c, s = small_case(name), host_scenes[name]
    pos = c["pos"]
    free = closest_model(pos, c["wv"])
    for md2 in (None, cs.radius_mix(free["dist2"], 5)):
        model = free if md2 is None else closest_model(pos, c["wv"], md2)
        host = s.closest_host(pos, md2)
        for use_bvh in (False, True):
            got = s.nearest_host(pos, 1, md2, use_bvh=use_bvh)
            for k in SLOTS:
                np.testing.assert_array_equal(got[k][:, 0].view(np.uint32), model[k].view(np.uint32), err_msg=f"{name} {k} vs closest_model")
                np.testing.assert_array_equal(got[k][:, 0].view(np.uint32), host[k].view(np.uint32), err_msg=f"{name} {k} vs closest_host")
            np.testing.assert_array_equal(got["count"], (model["tri"] != NO_TRI).astype(np.uint32))


@pytest.mark.parametrize("use_bvh", [False, True])
@pytest.mark.parametrize("name", SMALL)
def test_pages_of_two_equal_one_call_of_eight(host_scenes, name, use_bvh):
    """Four pages of 2, every point continued with the key of its last slot, equal k = 8 — free and within 0.25 scene scales, where
    many points are exhausted early: their last slot is the miss, a key behind which nothing counts, and their later pages stay misses."""
    c, s = small_case(name), host_scenes[name]
    call = lambda pos, k, md2, key: s.nearest_host(pos, k, md2, key, use_bvh=use_bvh)
    same(paged(call, c["pos"], 2, 4), nearest_model(c["table"], 8), f"{name} pages of 2")
    md2 = ns.squared_radius(c["scale"], 0.25, len(c["pos"]))
    want = nearest_model(c["table"], 8, md2)
    same(paged(call, c["pos"], 2, 4, md2), want, f"{name} pages of 2 within 0.25 scales")
    if name == "cornell":
        assert (want["count"] < 8).mean() > 0.5 and (want["count"] == 8).mean() > 0.3


def test_closest_all_is_the_sorted_table_within_the_radius(host_scenes):
    """closest_all's paging (through the host brute force on a host-only scene) on the Cornell box within 0.25 scene scales: the
    concatenated pages are exactly the set {j : dist2_j <= r^2} of the table in (dist2, index) order, up to 89 per point; max_items cuts
    each point's list; triangles_within is its offsets and indices."""
    c, s = small_case("cornell"), host_scenes["cornell"]
    pos, tab = c["pos"], c["table"]
    T, n = tab["dist2"].shape
    radius = f32(0.25 * c["scale"])
    md2 = ns.squared_radius(c["scale"], 0.25, n)
    want = nearest_model(tab, T, md2)
    np.testing.assert_array_equal(want["count"], (tab["dist2"] <= md2[None, :]).sum(0))
    off, d2, u, v, tri = s.closest_all(pos, radius)
    np.testing.assert_array_equal(np.diff(off), want["count"])
    assert want["count"].max() > 8 * 8 and (want["count"] == 0).any()
    filled = np.arange(T)[None, :] < want["count"][:, None]
    for k, a in zip(SLOTS, (d2, u, v, tri)):
        np.testing.assert_array_equal(a.view(np.uint32), want[k][filled].view(np.uint32), err_msg=k)
    assert off.dtype == np.int64 and d2.dtype == f32 and tri.dtype == np.uint32
    for i in (0, 7, 100):  # as sets, from the table alone
        assert set(tri[off[i]:off[i + 1]]) == set(np.flatnonzero(tab["dist2"][:, i] <= md2[i]))
    off5, d5, _, _, tri5 = s.closest_all(pos, np.full(n, radius, f32), page=3, max_items=5)
    first5 = np.arange(T)[None, :] < np.minimum(want["count"], 5)[:, None]
    np.testing.assert_array_equal(np.diff(off5), np.minimum(want["count"], 5))
    np.testing.assert_array_equal(d5, want["dist2"][first5])
    np.testing.assert_array_equal(tri5, want["tri"][first5])
    woff, wtri = bake.triangles_within(s, pos, radius)
    np.testing.assert_array_equal(woff, off)
    np.testing.assert_array_equal(wtri, tri)


@pytest.mark.parametrize("use_bvh", [False, True])
def test_radius_edges(host_scenes, use_bvh):
    """A radius exactly on the k-th entry's dist2 counts it and the next float below does not; negative radii count nothing, -0.0 admits
    dist2 == 0 alone, +inf is no radius, and a NaN radius counts nothing on the diagnostic (the entry points reject the entry)."""
    c, s = small_case("cornell"), host_scenes["cornell"]
    pos, tab = c["pos"], c["table"]
    n, k = len(pos), 3
    free = nearest_model(tab, 8)
    dk = np.ascontiguousarray(free["dist2"][:, k - 1])
    on = s.nearest_host(pos, 8, dk, use_bvh=use_bvh)
    same(on, nearest_model(tab, 8, dk), "radius on the third entry")
    assert (on["count"] >= k).all() and (on["dist2"][:, k - 1] == dk).all()
    below = np.nextafter(dk, f32(-np.inf))
    got = s.nearest_host(pos, 8, below, use_bvh=use_bvh)
    same(got, nearest_model(tab, 8, below), "radius just below the third entry")
    assert (got["count"] < k).all()
    with np.errstate(invalid="ignore"):
        assert (got["dist2"][got["tri"] != NO_TRI] < np.repeat(dk, 8).reshape(-1, 8)[got["tri"] != NO_TRI]).all()
    same(s.nearest_host(pos, 8, np.full(n, np.inf, f32), use_bvh=use_bvh), free, "radius +inf")
    for md in (f32(-1), f32(-np.inf), f32(np.nan)):
        got = s.nearest_host(pos, 8, np.full(n, md, f32), use_bvh=use_bvh)
        assert (got["count"] == 0).all() and (got["tri"] == NO_TRI).all() and np.isinf(got["dist2"]).all() and (got["u"] == 0).all(), md
    v = np.ascontiguousarray(c["wv"].reshape(-1, 3)[:200])
    both = np.concatenate([v, pos])
    mz = s.nearest_host(both, 8, np.full(len(both), -0.0, f32), use_bvh=use_bvh)
    same(mz, nearest_model(ns.candidate_table(c["wv"], both), 8, np.full(len(both), -0.0, f32)), "-0.0")
    assert (mz["count"][:200] >= 1).all() and (mz["dist2"][mz["tri"] != NO_TRI] == 0).all()
    assert ((mz["count"][200:] == 0) == (free["dist2"][:, 0] != 0)).all()


@pytest.mark.parametrize("use_bvh", [False, True])
def test_key_edges(host_scenes, use_bvh):
    """On the duplicates (ties on every point): the key (d_j, j) excludes j and keeps the tied j' > j; (d_j, j - 1) keeps j;
    after_dist2 = -inf excludes nothing; the miss slot (+inf, 0xFFFFFFFF) is a key behind which nothing counts; a NaN key counts nothing
    on the host diagnostic."""
    c, s = small_case("duplicates"), host_scenes["duplicates"]
    pos, tab = c["pos"], c["table"]
    n = len(pos)
    full = nearest_model(tab, 8)
    d0, j0 = np.ascontiguousarray(full["dist2"][:, 0]), np.ascontiguousarray(full["tri"][:, 0])
    assert (full["dist2"][:, 1] == d0).all() and (full["tri"][:, 1] > j0).all()  # the first two slots tie
    run = lambda after: s.nearest_host(pos, 8, None, after, use_bvh=use_bvh)
    got = run((d0, j0))
    same(got, nearest_model(tab, 8, None, (d0, j0)), "key on the first entry")
    np.testing.assert_array_equal(got["tri"][:, 0], full["tri"][:, 1])
    assert (got["dist2"][:, 0] == d0).all() and not (got["tri"] == j0[:, None]).any()
    has_prev = j0 > 0
    assert has_prev.sum() > n // 2
    prev = (d0, np.where(has_prev, j0 - 1, 0).astype(np.uint32))
    got = run(prev)
    same(got, nearest_model(tab, 8, None, prev), "key one index below the first entry")
    np.testing.assert_array_equal(got["tri"][has_prev, 0], j0[has_prev])
    same(run((np.full(n, -np.inf, f32), np.full(n, NO_TRI, np.uint32))), full, "after_dist2 = -inf")
    got = run((np.full(n, np.nan, f32), np.zeros(n, np.uint32)))
    assert (got["count"] == 0).all() and (got["tri"] == NO_TRI).all()
    same(got, nearest_model(tab, 8, None, (np.full(n, np.nan, f32), np.zeros(n, np.uint32))), "NaN key")
    for key_tri in (0, NO_TRI):
        assert (run((np.full(n, np.inf, f32), np.full(n, key_tri, np.uint32)))["count"] == 0).all()


# ---- the walk: the moving bound and the de-duplication on every tree -----------------------------------------------------------------------
def _walk_scenes():
    from test_scene_update import chain_scene
    return {
        "atrium_sah": lambda lib: Scene(scenes.get_scene("atrium", detail=1), -1, abi.RT_BVH_SAH, lib=lib),
        "atrium_lbvh": lambda lib: Scene(scenes.get_scene("atrium", detail=1), -1, abi.RT_BVH_LBVH, lib=lib),
        "median": lambda lib: Scene(chain_scene(), -1, abi.RT_BVH_LBVH, lib=lib),
        "offset_near": lambda lib: Scene(cs.offset_scene(cs.OFFSETS[0]), -1, abi.RT_BVH_SAH, lib=lib),
        "offset_far": lambda lib: Scene(cs.offset_scene(cs.OFFSETS[1]), -1, abi.RT_BVH_LBVH, lib=lib),
    }


def hold_walk(s, pos, what, ks=(1, 3, 8)):
    """walk == brute force for every k of ks free, and for k = 3 under the radius and key mix -> the brute force's free k = 8 answer"""
    free = None
    for k in ks:
        brute = s.nearest_host(pos, k)
        same(s.nearest_host(pos, k, use_bvh=True), brute, f"{what} k={k}")
        free = brute
    md2, after = key_mix(free, 3)
    brute = s.nearest_host(pos, 3, md2, after)
    same(s.nearest_host(pos, 3, md2, after, use_bvh=True), brute, f"{what} radius and key mix")
    assert (brute["count"] == 0).any() and (brute["count"] == 3).any()
    return free


@pytest.mark.parametrize("case", ["atrium_sah", "atrium_lbvh", "median", "offset_near", "offset_far"])
def test_the_walk_equals_the_brute_force_on_every_builder(devlib, case):
    """rt_scene_nearest_host: use_bvh = 1 (the kernel's cull against the moving bound on the decoded boxes) == use_bvh = 0 bit for bit,
    for k = 1, 3 and 8, free and under the radius and key mix, under SAH, LBVH and the median fallback (chain_scene: 41 equal triangles,
    lists full of ties), and on the atrium at detail 1 moved to (1000, -2000, 500) and to (1e5, 1e5, 1e5)."""
    s = _walk_scenes()[case](devlib)
    built = {"atrium_sah": abi.RT_BVH_SAH, "offset_near": abi.RT_BVH_SAH, "median": abi.RT_BVH_MEDIAN_INTERNAL}.get(case, abi.RT_BVH_LBVH)
    assert s.tree()["built_by"] == built
    s.check_bvh()
    n = 2048 if case == "median" else 512
    pos = point_mix(s.desc, n, 11)
    free = hold_walk(s, pos, case)
    assert (free["count"] == 8).all()
    walk = s.nearest_host(pos, 8, use_bvh=True)
    assert walk["node_visits"] < n * s.info().n_nodes or s.info().n_nodes < 64
    s.close()


def test_pre_split_triangles_are_listed_once_and_no_nan_is_listed(devlib):
    """closest_scenes.mixed_scene() under SAH: the two scene-spanning triangles are pre-split and sit whole in many leaves; 100 degenerate
    triangles give NaN candidates. The walk equals the brute force on every point — this query has no conditioning limit —, and the brute
    force the model; no list holds an index twice or a NaN; and the model over the LEAF RECORDS with the de-duplication left out lists a
    triangle twice, so a kernel without it could not pass."""
    sd, mask = cs.mixed_scene()
    s = Scene(sd, -1, abi.RT_BVH_SAH, lib=devlib)
    assert s.info().n_split_triangles > 0
    s.check_bvh()
    pos = point_mix(sd, 2048, 7)
    wv = world_vertices(sd)
    tab = ns.candidate_table(wv, pos)
    assert np.isnan(tab["dist2"]).any()
    free = hold_walk(s, pos, "mixed sah", ks=(1, 2, 4, 8))
    same(free, nearest_model(tab, 8), "mixed sah: brute force vs model")
    md2, after = key_mix(free, 9)
    same(s.nearest_host(pos, 4, md2, after), nearest_model(tab, 4, md2, after), "mixed sah: brute force vs model, mix")
    assert not np.isnan(free["dist2"]).any() and (free["count"] == 8).all()
    srt = np.sort(free["tri"], 1)
    assert not (srt[:, 1:] == srt[:, :-1]).any()
    gi = s.tree()["global_index"]
    split = np.flatnonzero(np.bincount(gi, minlength=len(wv)) > 1)
    assert len(split) >= 2
    listed = np.isin(free["tri"], split)
    assert listed.any(1).sum() > 50 and (np.isin(free["tri"], np.flatnonzero(mask))).any()  # pre-split and degenerate triangles are in lists
    pts = np.flatnonzero(listed.any(1))[:64]
    recs = {k: a[gi][:, pts] for k, a in tab.items()}
    with_dups = nearest_model(recs, 8, index=gi)
    once = nearest_model({k: a[:, pts] for k, a in tab.items()}, 8)
    same({k: free[k][pts] for k in ns.OUTPUTS}, once, "the walk's lists on these points")
    assert not np.array_equal(with_dups["tri"], once["tri"])
    assert (with_dups["tri"][:, 1:] == with_dups["tri"][:, :-1]).any(1).all()
    s.close()


@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_the_full_pile_under_a_moving_bound(devlib, builder):
    """8,192 parallel triangles in one box, stack_need > 12: the walk equals the brute force, and with k = 8 it visits fewer nodes and
    tests fewer triangles than the same walk with a list that never fills (k = the triangle count: the bound stays at max_dist2)."""
    sd = cs.pile_scene()
    s = Scene(sd, -1, cs.BUILDERS[builder], lib=devlib)
    assert s.tree()["stack_need"] > cs.K_LDS_STACK
    pos = np.concatenate([point_mix(sd, 384, 1), cs.pile_corner_points(128, 2)])
    hold_walk(s, pos, f"pile {builder}")
    few = np.ascontiguousarray(pos[::16])  # (a list of 8,192 costs the host walk its length per candidate: 32 points)
    moving = s.nearest_host(few, 8, use_bvh=True)
    held = s.nearest_host(few, 8192, use_bvh=True, slots=False)
    assert (held["count"] == 8192).all()
    print(f"pile {builder}, {len(few)} points: k = 8 {moving['node_visits']} node visits, {moving['tri_tests']} triangle tests; "
          f"bound held at max_dist2 {held['node_visits']} and {held['tri_tests']}")
    assert moving["node_visits"] < held["node_visits"] and moving["tri_tests"] < held["tri_tests"]
    s.close()


def test_the_bound_moves_up_with_k(devlib):
    """The atrium at detail 1: the walk's node visits and triangle tests grow with k (1, 2, 4, 8) and stay under the walk with the bound
    held at max_dist2 — the figures DESIGN.md §25 quotes are printed here."""
    s = Scene(scenes.get_scene("atrium", detail=1), -1, abi.RT_BVH_SAH, lib=devlib)
    pos = point_mix(s.desc, 2048, 21)
    n = len(pos)
    rows = [s.nearest_host(pos, k, use_bvh=True, slots=False) for k in (1, 2, 4, 8)]
    few = 8  # (a list that never fills costs the host walk its length per candidate; it visits every node and record for every point)
    held = s.nearest_host(pos[:few], s.info().n_triangles, use_bvh=True, slots=False)
    assert (held["count"] == s.info().n_triangles).all()
    held = {k: held[k] * (n // few) for k in ("node_visits", "tri_tests")}
    assert held["node_visits"] == n * s.info().n_nodes and held["tri_tests"] == n * s.info().n_leaf_records
    one = s.closest_host(pos, use_bvh=True)
    assert (rows[0]["node_visits"], rows[0]["tri_tests"]) == (one["node_visits"], one["tri_tests"])  # k = 1 is k_closest's walk
    for k, r in zip((1, 2, 4, 8), rows):
        print(f"atrium detail 1, k={k}: {r['node_visits'] / n:.1f} node visits and {r['tri_tests'] / n:.1f} triangle tests per point")
    print(f"bound held at max_dist2: {held['node_visits'] / n:.1f} and {held['tri_tests'] / n:.1f}")
    v = [r["node_visits"] for r in rows] + [held["node_visits"]]
    t = [r["tri_tests"] for r in rows] + [held["tri_tests"]]
    assert v == sorted(v) and t == sorted(t) and v[3] < 0.1 * v[4]
    s.close()


# ---- above the ABI -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_contact_points_re_form_the_point_and_dist2(host_scenes, name):
    """contact_points with k = 1 equals rt_scene_closest_host's `point` bit for bit, NaN on a miss; for k = 8 the recomputed r = p - ... has
    dot(r, r) equal to the listed dist2 bit for bit: why the query needs no point output."""
    c, s = small_case(name), host_scenes[name]
    pos, wv = c["pos"], c["wv"]
    md2 = cs.radius_mix(s.closest_host(pos)["dist2"], 5)
    for m in (None, md2):
        one, ref = s.nearest_host(pos, 1, m), s.closest_host(pos, m)
        got = bake.contact_points(wv, pos, one["u"][:, 0], one["v"][:, 0], one["tri"][:, 0])
        np.testing.assert_array_equal(got.view(np.uint32), ref["point"].view(np.uint32))
    assert np.isnan(got).any() and not np.isnan(got).all()
    out = s.nearest_host(pos, 8)
    pts = bake.contact_points(wv, pos, out["u"], out["v"], out["tri"])
    assert pts.shape == (len(pos), 8, 3) and pts.dtype == f32
    w = wv[out["tri"].astype(np.int64)]
    ap = pos[:, None, :] - w[..., 0, :]
    r = (ap - out["u"][..., None] * (w[..., 1, :] - w[..., 0, :])) - out["v"][..., None] * (w[..., 2, :] - w[..., 0, :])
    d2 = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
    assert d2.dtype == f32
    np.testing.assert_array_equal(d2.view(np.uint32), out["dist2"].view(np.uint32))
    np.testing.assert_array_equal(pts.view(np.uint32), (pos[:, None, :] - r).view(np.uint32))


# ---- what the unit relies on in texts it does not own --------------------------------------------------------------------------------------
def test_what_the_kernel_relies_on_in_the_point_traversal(devlib):
    """rt_nearest.hip opens a point's list at the step that finds cur == 0 and carries k and the key to it in T.best.u / v / tri. That
    holds while (1) closest_begin is the only text of rt_closest_step.h that sets cur to the root, (2) no node has the root as a child, so
    no push, descent or pop brings cur back to 0, and (3) closest_inner reads nothing of T.best but best.t and writes none of it."""
    src = (CSRC / "rt_closest_step.h").read_text()
    body = lambda name: re.search(rf"^RT_DEV void {name}\(.*?^}}", src, re.M | re.S).group(0)
    assert len(re.findall(r"\bcur = 0;", src)) == 1 and "T.cur = 0;" in body("closest_begin")
    inner = re.sub(r"//.*", "", body("closest_inner"))
    assert set(re.findall(r"\bbest\.\w+", inner)) == {"best.t"} and not re.search(r"\bbest\.t\s*=[^=]", inner) and "T.best" in inner
    assert not re.search(r"[(,]\s*T\.best\s*[,)]", inner)  # nor handed on whole
    unit = (CSRC / "rt_nearest.hip").read_text()
    assert "closest_inner(" in unit and "closest_begin(" in unit and "closest_point_on_record(" in unit and "hit_list_insert<" in unit
    assert "query_frame<" in unit and "asm" not in unit and "global_load_dwordx4 %" not in unit  # nothing of the traversal restated
    closest = (CSRC / "rt_closest.hip").read_text()
    # the list's store and the whole-leaf read have one text each (rt_hit_list.h, rt_whole_leaf.h), no second one in a unit
    multi = (CSRC / "rt_multihit.hip").read_text()
    assert "store_slot" not in unit and "store_slot" not in multi
    assert "tri_ld4(" not in unit and "tri_ld4(" not in multi and "tri_ld4(" not in closest
    assert "store_slot" in (CSRC / "rt_hit_list.h").read_text() and "tri_ld4(" in (CSRC / "rt_whole_leaf.h").read_text()
    assert "rt_closest_step.h" in closest and "void closest_inner" not in closest and "void closest_begin" not in closest  # one text
    from test_scene_update import chain_scene
    for sd, builder in ((cs.mixed_scene()[0], abi.RT_BVH_SAH), (scenes.get_scene("cornell"), abi.RT_BVH_LBVH), (chain_scene(), abi.RT_BVH_LBVH)):
        s = Scene(sd, -1, builder, lib=devlib)
        nodes = s.tree()["nodes"]
        assert len(nodes) > 1 and (nodes[:, 12:16].view(np.int32) != 0).all()  # child words: >= 0 an inner node's index, and never the root's
        s.close()


# ---- the listing ---------------------------------------------------------------------------------------------------------------------------
def _k_nearest(n):
    return f"_ZN2rt9k_nearestILj{n}EEEvNS_8SceneDevENS_10NearestDevE"


def test_nearest_kernels_have_the_resources_design_states(tmp_path):
    """k_nearest<2>, <4>, <8> (rt_nearest.hip): registers, spills, scratch, LDS and occupancy are the figures of DESIGN.md §25, read from
    the listing and from DESIGN.md itself. No VGPR is spilled and the scratch is exactly the frame every RT_TRAVERSAL_LDS kernel has
    (k_query's: the traversal stack's spill array): the lists live in registers. The node fetch is closest_inner's plain loads, so the ISA
    hazard scan of the asm-issued fetch has nothing to look at here."""
    from test_denoise import _listing
    from test_svgf import _metadata
    lines = _listing("rt_nearest.hip", tmp_path)
    meta = "\n".join(lines)
    design = (REPO / "DESIGN.md").read_text()
    kq = _metadata("\n".join(_listing("rt_query.hip", tmp_path)), "_ZN2rt7k_queryILb0EEEvNS_8SceneDevENS_8QueryDevE", "private_segment_fixed_size")
    assert kq == 224
    names = re.findall(r"^(_ZN2rt9k_nearestILj\dE\S+):", meta, re.M)
    occs = [int(x) for x in re.findall(r"^; Occupancy: (\d+)", meta, re.M)]
    assert len(names) == 3 and len(occs) == 3  # three kernels in the unit, in the listing's order
    occ = dict(zip(names, occs))
    for n in (2, 4, 8):
        sym = _k_nearest(n)
        got = {k: _metadata(meta, sym, k) for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size",
                                                    "group_segment_fixed_size")}
        got["occupancy"] = occ[sym]
        m = re.search(rf"`k_nearest<{n}>`: (\d+) VGPRs, (\d+) SGPRs, (\d+) VGPRs spilled, (\d+) bytes of scratch per lane, ([\d,]+) bytes of LDS "
                      r"per workgroup, (\d+) waves per SIMD", design)
        assert m, f"DESIGN.md states k_nearest<{n}>'s resources in one sentence"
        stated = {"vgpr_count": int(m.group(1)), "sgpr_count": int(m.group(2)), "vgpr_spill_count": int(m.group(3)),
                  "private_segment_fixed_size": int(m.group(4)), "group_segment_fixed_size": int(m.group(5).replace(",", "")),
                  "occupancy": int(m.group(6))}
        assert got == stated, n
        assert got["vgpr_spill_count"] == 0 and got["private_segment_fixed_size"] == kq
        assert got["vgpr_count"] * got["occupancy"] <= 512 and (got["occupancy"] // 2) * got["group_segment_fixed_size"] <= 160 * 1024
    # the only scratch instructions are the spill array's, addressed by the entry's register, never a spill slot's constant offset
    scratch = [ln.strip() for ln in lines if re.match(r"\s+scratch_", ln)]
    assert scratch and all(re.fullmatch(r"scratch_(load|store)_dword v\d+, v\d+, off", ln) for ln in scratch), scratch
