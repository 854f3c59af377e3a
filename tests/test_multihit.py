"""Multi-hit ray queries (include/rt_mi355x.h: rt_trace_rays_multi[_device], rt_scene_multihit_host) without a GPU: the exported entry
points and the struct layout, the refusals in front of the device, the Python wrappers, the host brute force against the oracle-table
model (tests/multihit_scenes.py) on the three small scenes, the k = 1, paging and exhaustion identities, tmax and key edges, the host walk
of the tree (the kernel's moving bound and de-duplication) against the brute force on every builder, what the bound saves on the full
pile, trace_all / crossings / inside_mask on the cube, and the kernel's listing: resources as DESIGN.md §24 states them, hazard scan."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import multihit_scenes as ms
from multihit_scenes import aimed_rays, counting, hits_per_ray, multihit_model, same, small_case
from rtamd import abi, bake, scenes
from rtamd.renderer import Scene
from test_closest_points import NO_TRI, tri_scene

REPO = Path(__file__).resolve().parent.parent
f32 = np.float32
K_NEAR = f32(0.0001)  # rt_types.h: kTNear
FIELDS = ["n", "k", "org", "dir", "tmax", "after_t", "after_tri", "t", "u", "v", "tri", "count"]
SLOTS = ("t", "u", "v", "tri")


# ---- the surface --------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_prototyped(rtlib, devlib, tmp_path):
    header = (REPO / "include" / "rt_mi355x.h").read_text()
    assert "typedef struct rt_multihit_query {" in header and "#define RT_MULTIHIT_MAX 8" in header and abi.RT_MULTIHIT_MAX == 8
    for name in ("rt_trace_rays_multi", "rt_trace_rays_multi_device"):
        assert re.search(rf"^int {name}\(rt_scene\* scene, const rt_multihit_query\* q", header, re.M), name
    assert re.search(r"^int rt_scene_multihit_host\(const rt_scene\* scene, uint32_t n, uint32_t k, const float\* org, const float\* dir", header, re.M)
    for name in ("rt_trace_rays_multi", "rt_trace_rays_multi_device", "rt_scene_multihit_host"):
        assert name in abi.PROTOTYPES
        for lib in (rtlib, devlib):
            assert hasattr(lib, name), name
    assert [f[0] for f in abi.rt_multihit_query._fields_] == FIELDS
    assert rtlib.rt_abi_version() == 8 and "#define RT_ABI_VERSION 8" in header
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_mi355x.h"\nint main(void){printf("%zu\\n", sizeof(rt_multihit_query));' +
                   "".join(f'printf("%zu\\n", offsetof(rt_multihit_query, {f}));' for f in FIELDS) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", str(REPO / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(abi.rt_multihit_query)] + [getattr(abi.rt_multihit_query, f).offset for f in FIELDS]
    assert got[0] == 88


def _query(n=4, k=2, keep=None, **want):
    bufs = {"org": np.zeros((4, 3), f32), "dir": np.ones((4, 3), f32), "tmax": np.ones(4, f32), "after_t": np.zeros(4, f32),
            "after_tri": np.zeros(4, np.uint32), "t": np.zeros((4, 8), f32), "u": np.zeros((4, 8), f32), "v": np.zeros((4, 8), f32),
            "tri": np.zeros((4, 8), np.uint32), "count": np.zeros(4, np.uint32)}
    if keep is not None:
        keep.append(bufs)
    q = abi.rt_multihit_query(n=n, k=k)
    for name in FIELDS[2:]:
        setattr(q, name, bufs[name].ctypes.data if want.get(name, True) else None)
    return q


@pytest.mark.parametrize("entry", ["rt_trace_rays_multi", "rt_trace_rays_multi_device"])
def test_refusals_come_in_order_and_before_any_device_call(rtlib, entry):
    """On a host-only scene every status was decided in front of the device, in query_check's order: RT_ERR_INVALID for a NULL scene or
    query; RT_OK for n == 0 whatever else is wrong; RT_ERR_INVALID for k outside 1 .. 8, then NULL org or dir, then half a key, then every
    output NULL; RT_ERR_NO_DEVICE last."""
    s = Scene(scenes.get_scene("cornell"), device=-1)
    fn = getattr(rtlib, entry)
    call = (lambda h, q: fn(h, q)) if entry == "rt_trace_rays_multi" else (lambda h, q: fn(h, q, None))
    err = lambda: rtlib.rt_last_error().decode()
    keep = []
    inv = abi.RT_ERR_INVALID
    none = {k: False for k in ms.OUTPUTS}
    assert call(None, C.byref(_query(keep=keep))) == inv and "null argument" in err()
    assert call(s.h, None) == inv and "null argument" in err()
    assert call(s.h, C.byref(_query(n=0, keep=keep))) == abi.RT_OK
    assert call(s.h, C.byref(_query(n=0, k=0, keep=keep, org=False, after_t=False, **none))) == abi.RT_OK
    for k in (0, 9, 0xFFFFFFFF):
        assert call(s.h, C.byref(_query(k=k, keep=keep))) == inv and "k must be" in err()
        assert call(s.h, C.byref(_query(k=k, keep=keep, org=False, after_tri=False, **none))) == inv and "k must be" in err()  # k first
    for kw in ({"org": False}, {"dir": False}):
        assert call(s.h, C.byref(_query(keep=keep, **kw))) == inv and "org or dir" in err()
        assert call(s.h, C.byref(_query(keep=keep, after_t=False, **kw, **none))) == inv and "org or dir" in err()  # before the key
    for kw in ({"after_t": False}, {"after_tri": False}):
        assert call(s.h, C.byref(_query(keep=keep, **kw))) == inv and "key" in err()
        assert call(s.h, C.byref(_query(keep=keep, **kw, **none))) == inv and "key" in err()  # the key before the outputs
    assert call(s.h, C.byref(_query(keep=keep, **none))) == inv and "output" in err()
    for kw in ({}, {"tmax": False}, {"after_t": False, "after_tri": False}, {"t": False, "u": False, "v": False, "tri": False}, {"count": False},
               {"k": 1}, {"k": 8}):
        assert call(s.h, C.byref(_query(keep=keep, **kw))) == abi.RT_ERR_NO_DEVICE, kw
        assert "host-only" in err()
    # what the host form refuses per ray comes after the device test: a host-only scene never gets that far
    bad = _query(keep=keep)
    keep[-1]["after_t"][1] = np.nan
    assert call(s.h, C.byref(bad)) == abi.RT_ERR_NO_DEVICE
    s.close()


def test_python_wrappers_refuse_wrong_shapes_and_dtypes(rtlib):
    s = Scene(scenes.get_scene("cube"), device=-1)
    org, d = np.zeros((2, 3), f32), np.ones((2, 3), f32)
    with pytest.raises(abi.RtError) as e:
        s.trace_multi(org, d, 2)
    assert e.value.status == abi.RT_ERR_NO_DEVICE
    key = (np.zeros(2, f32), np.zeros(2, np.uint32))
    bad = [dict(org=np.zeros(6, f32)), dict(org=np.zeros((2, 4), f32)), dict(dirs=np.ones((3, 3), f32)), dict(k=0), dict(k=9), dict(k=2.0),
           dict(k=True), dict(tmax=np.ones(3, f32)), dict(tmax=np.ones((2, 1), f32)), dict(tmax=np.array(["a", "b"])), dict(after=key[0]),
           dict(after=(key[0],)), dict(after=(key[0], np.zeros(2, f32))), dict(after=(np.zeros(2, np.int32), key[1])),
           dict(after=(np.zeros(3, f32), np.zeros(3, np.uint32)))]
    for kw in bad:
        args = dict(org=org, dirs=d, k=2)
        args.update(kw)
        with pytest.raises(ValueError):
            s.trace_multi(**args)
        if kw.get("k") != 9:  # (the host diagnostic takes any k >= 1)
            with pytest.raises(ValueError):
                s.multihit_host(**args)
    for kw in (dict(page=0), dict(page=9), dict(max_hits=0), dict(max_hits=1.5), dict(tmax=np.ones(3, f32))):
        with pytest.raises(ValueError):
            s.trace_all(org, d, **kw)
    out = s.multihit_host(np.zeros((0, 3), f32), np.zeros((0, 3), f32), 3)
    assert out["t"].shape == (0, 3) and out["tri"].dtype == np.uint32 and out["count"].shape == (0,)
    with pytest.raises(abi.RtError) as e:
        s.trace_multi_device(5, 2, 0, 0)
    assert e.value.status == abi.RT_ERR_INVALID
    with pytest.raises(ValueError):
        bake.inside_mask(s, np.zeros((2, 2), f32), (0, 0, 1))
    with pytest.raises(ValueError):
        bake.inside_mask(s, org, (0, 1))
    host = rtlib.rt_scene_multihit_host
    o, dd = abi.fptr(org), abi.fptr(d)
    assert host(None, 0, 1, None, None, None, None, None, 0, None, None, None, None, None, None, None) == abi.RT_ERR_INVALID
    assert host(s.h, 1, 1, None, dd, None, None, None, 0, None, None, None, None, None, None, None) == abi.RT_ERR_INVALID
    assert host(s.h, 1, 1, o, dd, None, None, None, 2, None, None, None, None, None, None, None) == abi.RT_ERR_INVALID
    assert host(s.h, 1, 0, o, dd, None, None, None, 0, None, None, None, None, None, None, None) == abi.RT_ERR_INVALID
    assert host(s.h, 1, 1, o, dd, None, abi.fptr(key[0]), None, 0, None, None, None, None, None, None, None) == abi.RT_ERR_INVALID
    assert host(s.h, 2, 40, o, dd, None, None, None, 1, None, None, None, None, None, None, None) == abi.RT_OK  # every output NULL, k > 8
    s.close()


# ---- the three small scenes: the brute force is the oracle's table -------------------------------------------------------------------------
def test_the_small_scenes_meet_the_conditions_their_tests_lean_on():
    """Cornell: at least 70 % of the rays have two or more counting hits. The duplicates: every ray has a tie that straddles slot k - 1 for
    every k tested (1, 2, 3, 8 here; 1 .. 8 on the device). The pile of 256: at least half of the rays fill 8 slots and have more behind."""
    c = hits_per_ray(small_case("cornell")["table"])
    print(f"cornell: {100.0 * (c >= 2).mean():.1f} % of the rays have >= 2 hits, at most {c.max()} per ray")
    assert (c >= 2).mean() >= 0.70
    dup = small_case("duplicates")["table"]
    print(f"duplicates: at least {hits_per_ray(dup).min()} hits per ray")
    for k in range(1, 9):
        assert ms.tie_straddles(dup, k).all() == (k != 7), k  # seven-fold ties: a list of 7 ends where a group ends ...
        assert ms.tie_straddles(dup, k, ms.first_hit_key(dup)).all() == (k != 6), k  # ... and behind the first hit's key a list of 6 does
        assert len(ms.duplicate_runs(dup, k)) == 2
    p = hits_per_ray(small_case("pile256")["table"])
    print(f"pile256: {100.0 * (p >= 9).mean():.1f} % of the rays have >= 9 hits, at most {p.max()} per ray")
    assert (p >= 9).mean() >= 0.5


@pytest.fixture(scope="module")
def host_scenes(rtlib):
    made = {name: Scene(small_case(name)["sd"], device=-1) for name in ("cornell", "duplicates", "pile256")}
    yield made
    for s in made.values():
        s.close()


@pytest.mark.parametrize("name", ["cornell", "duplicates", "pile256"])
def test_the_brute_force_equals_the_oracle_table_model(host_scenes, name):
    """multihit_host(use_bvh = 0) == multihit_model on the oracle's one-triangle table for k = 1, 2, 3 and 8, with no tmax and with a tmax
    on every ray's second hit (where it has one), and the host walk equals both."""
    c, s = small_case(name), host_scenes[name]
    full = multihit_model(c["table"], 2)
    tm = np.where(full["count"] == 2, full["t"][:, 1], f32(np.inf)).astype(f32)
    for k in (1, 2, 3, 8):
        for tmax in (None, tm):
            want = multihit_model(c["table"], k, tmax)
            same(s.multihit_host(c["org"], c["dirs"], k, tmax), want, f"{name} k={k} brute force")
            same(s.multihit_host(c["org"], c["dirs"], k, tmax, use_bvh=True), want, f"{name} k={k} walk")
            filled = np.arange(k)[None, :] < want["count"][:, None]
            assert ((want["tri"] != NO_TRI) == filled).all() and np.isinf(want["t"][~filled]).all()
        if name == "duplicates":  # the run of this k whose tie straddles slot k - 1 on every ray (multihit_scenes.duplicate_runs)
            for what, after in ms.duplicate_runs(c["table"], k):
                want = multihit_model(c["table"], k, None, after)
                same(s.multihit_host(c["org"], c["dirs"], k, None, after), want, f"{name} k={k} {what} brute force")
                same(s.multihit_host(c["org"], c["dirs"], k, None, after, use_bvh=True), want, f"{name} k={k} {what} walk")


@pytest.mark.parametrize("name", ["cornell", "duplicates", "pile256"])
def test_k_1_is_the_closest_hit(host_scenes, oracle, name):
    """With k = 1 and no key the slot is the oracle's closest hit of the whole scene, bit for bit — and so is the table's per-ray minimum."""
    c, s = small_case(name), host_scenes[name]
    t, u, v, tri = oracle.OracleScene(c["sd"]).intersect(c["org"], c["dirs"], False)
    for use_bvh in (False, True):
        got = s.multihit_host(c["org"], c["dirs"], 1, use_bvh=use_bvh)
        for k, w in zip(SLOTS, (t, u, v, tri)):
            np.testing.assert_array_equal(got[k][:, 0], w, err_msg=f"{name} {k}")
        np.testing.assert_array_equal(got["count"], (tri != NO_TRI).astype(np.uint32))
    same({k: a[:, None] for k, a in zip(SLOTS, (t, u, v, tri))}, multihit_model(c["table"], 1), f"{name} table minimum", SLOTS)


def paged(call, org, dirs, page, pages):
    """`pages` pages of `page` hits, each continued with the key of its last slot for the rays that filled it; the others keep their miss
    slots. -> the pages side by side, (n, page * pages), and the total count"""
    n = len(org)
    out = {"t": np.full((n, page * pages), np.inf, f32), "u": np.zeros((n, page * pages), f32), "v": np.zeros((n, page * pages), f32),
           "tri": np.full((n, page * pages), NO_TRI, np.uint32), "count": np.zeros(n, np.uint32)}
    active, key = np.arange(n), None
    for p in range(pages):
        got = call(org[active], dirs[active], page, None, key)
        for k in SLOTS:
            out[k][active, p * page:(p + 1) * page] = got[k]
        out["count"][active] += got["count"]
        more = got["count"] == page
        key = (got["t"][more, page - 1], got["tri"][more, page - 1])
        active = active[more]
    return out, len(active)


@pytest.mark.parametrize("use_bvh", [False, True])
@pytest.mark.parametrize("name", ["cornell", "duplicates", "pile256"])
def test_pages_of_two_equal_one_call_of_eight(host_scenes, name, use_bvh):
    """Four pages of 2 continued with the key equal k = 8; a ray with count < 2 on a page is exhausted (its later pages stay misses)."""
    c, s = small_case(name), host_scenes[name]
    got, _ = paged(lambda *a: s.multihit_host(*a, use_bvh=use_bvh), c["org"], c["dirs"], 2, 4)
    same(got, multihit_model(c["table"], 8), f"{name} pages of 2")


def test_pages_until_exhaustion_are_the_sorted_table_on_the_pile(host_scenes):
    """trace_all's paging (pages of 8 through the host brute force on a host-only scene): the concatenated pages are every counting hit of
    the table in (t, index) order, up to 254 per ray; max_hits cuts each ray's list."""
    c, s = small_case("pile256"), host_scenes["pile256"]
    T = c["table"]["t"].shape[0]
    want = multihit_model(c["table"], T)
    off, t, u, v, tri = s.trace_all(c["org"], c["dirs"])
    np.testing.assert_array_equal(np.diff(off), want["count"])
    assert want["count"].max() > 100
    filled = np.arange(T)[None, :] < want["count"][:, None]
    for k, a in zip(SLOTS, (t, u, v, tri)):
        np.testing.assert_array_equal(a, want[k][filled], err_msg=k)
    off5, t5, _, _, tri5 = s.trace_all(c["org"], c["dirs"], page=3, max_hits=5)
    np.testing.assert_array_equal(np.diff(off5), np.minimum(want["count"], 5))
    first5 = np.arange(T)[None, :] < np.minimum(want["count"], 5)[:, None]
    np.testing.assert_array_equal(t5, want["t"][first5])
    np.testing.assert_array_equal(tri5, want["tri"][first5])


@pytest.mark.parametrize("use_bvh", [False, True])
def test_tmax_edges(host_scenes, use_bvh):
    """tmax = t_j counts hit j; the next float towards 0 does not; tmax <= kTNear, 0, negative and -inf find nothing; a NaN tmax counts
    nothing on the host diagnostic (the entry points reject the ray)."""
    c, s = small_case("cornell"), host_scenes["cornell"]
    full = multihit_model(c["table"], 8)
    has = full["count"] >= 2
    assert has.sum() > 1000
    org, d = c["org"][has], c["dirs"][has]
    t2 = full["t"][has, 1]
    tab = {k: a[:, has] for k, a in c["table"].items()}
    on = s.multihit_host(org, d, 8, t2, use_bvh=use_bvh)
    same(on, multihit_model(tab, 8, t2), "tmax on the second hit")
    assert (on["count"] >= 2).all() and (on["t"][:, 1] == t2).all()
    below = np.nextafter(t2, f32(0))
    got = s.multihit_host(org, d, 8, below, use_bvh=use_bvh)
    same(got, multihit_model(tab, 8, below), "tmax just below the second hit")
    assert (got["count"] < on["count"]).all() and (got["t"][got["tri"] != NO_TRI] < t2.repeat(8).reshape(-1, 8)[got["tri"] != NO_TRI]).all()
    for tm in (K_NEAR, f32(0), f32(-0.0), f32(-1), f32(-np.inf), f32(np.nan)):
        got = s.multihit_host(org, d, 8, np.full(len(org), tm, f32), use_bvh=use_bvh)
        assert (got["count"] == 0).all() and (got["tri"] == NO_TRI).all() and np.isinf(got["t"]).all() and (got["u"] == 0).all(), tm


@pytest.mark.parametrize("use_bvh", [False, True])
def test_key_edges(host_scenes, use_bvh):
    """On the duplicates (seven-fold ties): the key (t_j, j) excludes j and keeps the tied j' > j; (t_j, j - 1) keeps j; after_t = -inf
    excludes nothing; a NaN key counts nothing on the host diagnostic."""
    c, s = small_case("duplicates"), host_scenes["duplicates"]
    org, d, tab = c["org"], c["dirs"], c["table"]
    n = len(org)
    full = multihit_model(tab, 8)
    t0, j0 = full["t"][:, 0], full["tri"][:, 0]
    assert (full["t"][:, 1] == t0).all() and (full["tri"][:, 1] > j0).all()  # the first two slots tie
    run = lambda after: s.multihit_host(org, d, 8, None, after, use_bvh=use_bvh)
    got = run((t0, j0))
    same(got, multihit_model(tab, 8, None, (t0, j0)), "key on the first hit")
    np.testing.assert_array_equal(got["tri"][:, 0], full["tri"][:, 1])
    assert (got["t"][:, 0] == t0).all() and not (got["tri"] == j0[:, None]).any()
    has_prev = j0 > 0
    assert has_prev.sum() > n // 2
    prev = (t0, np.where(has_prev, j0 - 1, 0).astype(np.uint32))
    got = run(prev)
    same(got, multihit_model(tab, 8, None, prev), "key one index below the first hit")
    np.testing.assert_array_equal(got["tri"][has_prev, 0], j0[has_prev])
    same(run((np.full(n, -np.inf, f32), np.full(n, NO_TRI, np.uint32))), full, "after_t = -inf")
    got = run((np.full(n, np.nan, f32), np.zeros(n, np.uint32)))
    assert (got["count"] == 0).all() and (got["tri"] == NO_TRI).all()
    same(got, multihit_model(tab, 8, None, (np.full(n, np.nan, f32), np.zeros(n, np.uint32))), "NaN key")
    inf_key = run((np.full(n, np.inf, f32), np.zeros(n, np.uint32)))
    assert (inf_key["count"] == 0).all()


@pytest.mark.parametrize("use_bvh", [False, True])
def test_rays_with_nan_or_zero_direction_find_nothing(host_scenes, use_bvh):
    c, s = small_case("cornell"), host_scenes["cornell"]
    org = c["org"][:8].copy()
    d = c["dirs"][:8].copy()
    d[0], d[1], d[2, 1], d[3] = 0.0, np.nan, np.nan, -0.0
    got = s.multihit_host(org, d, 4, use_bvh=use_bvh)
    assert (got["count"][:4] == 0).all() and (got["tri"][:4] == NO_TRI).all() and np.isinf(got["t"][:4]).all()
    same({k: a[4:] for k, a in got.items() if k in ms.OUTPUTS}, multihit_model({k: a[:, 4:8] for k, a in c["table"].items()}, 4), "the others")


# ---- the walk: the moving bound and the de-duplication on every tree -----------------------------------------------------------------------
def _walk_scenes():
    from test_scene_update import chain_scene
    return {
        "atrium_sah": lambda lib: Scene(scenes.get_scene("atrium", detail=1), -1, abi.RT_BVH_SAH, lib=lib),
        "atrium_lbvh": lambda lib: Scene(scenes.get_scene("atrium", detail=1), -1, abi.RT_BVH_LBVH, lib=lib),
        "median": lambda lib: Scene(chain_scene(), -1, abi.RT_BVH_LBVH, lib=lib),
        "cornell_lbvh": lambda lib: Scene(scenes.get_scene("cornell"), -1, abi.RT_BVH_LBVH, lib=lib),
    }


def key_mix(free, seed):
    """per-ray tmax and key around the unbounded answer `free` (k >= 4): tmax on the third hit, just below it, +inf or -1; the key on the
    first hit, one index below it, none (-inf) or beyond everything (+inf)"""
    g = np.random.default_rng(seed)
    n = len(free["count"])
    t3 = np.where(free["count"] >= 3, free["t"][:, 2], f32(1.0)).astype(f32)
    kind = g.integers(0, 4, n)
    tmax = np.select([kind == 0, kind == 1, kind == 2], [t3, np.nextafter(t3, f32(0)), f32(np.inf)], f32(-1.0)).astype(f32)
    kk = g.integers(0, 4, n)
    hit = free["count"] >= 1
    t0 = np.where(hit, free["t"][:, 0], f32(0.5)).astype(f32)
    j0 = np.where(hit, free["tri"][:, 0], 0).astype(np.uint32)
    at = np.select([kk == 0, kk == 1, kk == 2], [t0, t0, f32(-np.inf)], f32(np.inf)).astype(f32)
    atri = np.where((kk == 1) & (j0 > 0), j0 - 1, j0).astype(np.uint32)
    return tmax, (at, atri)


@pytest.mark.parametrize("case", ["atrium_sah", "atrium_lbvh", "median", "cornell_lbvh"])
def test_the_walk_equals_the_brute_force_on_every_builder(devlib, case):
    """rt_scene_multihit_host: use_bvh = 1 (the kernel's bound rule on the decoded boxes) == use_bvh = 0 bit for bit on aimed rays, for
    k = 1, 3 and 8, free and under a tmax and key mix, on every builder a host-only scene can have: SAH, LBVH and the median fallback."""
    s = _walk_scenes()[case](devlib)
    tree = s.tree()
    assert tree["built_by"] == {"atrium_sah": abi.RT_BVH_SAH, "median": abi.RT_BVH_MEDIAN_INTERNAL}.get(case, abi.RT_BVH_LBVH)
    s.check_bvh()
    n = 512 if case.startswith("atrium") else 2048
    org, d = aimed_rays(s.desc, n, 11)
    if case == "median":  # half of the rays at the corner cell of the forty-one equal triangles (the others: at the unit cube, mostly misses)
        tgt = np.random.default_rng(5).uniform(0.0, 2.0 ** -23, (n // 2, 3)).astype(f32)
        d[n // 2:] = tgt - org[n // 2:]
    for k in (1, 3, 8):
        brute = s.multihit_host(org, d, k)
        walk = s.multihit_host(org, d, k, use_bvh=True)
        same(walk, brute, f"{case} k={k}")
        assert walk["node_visits"] < n * s.info().n_nodes or s.info().n_nodes < 64
        if k == 8:
            if case == "median":
                assert (brute["count"] == 8).sum() >= 16  # a hit there is 41 equal candidates: the list fills with ties
            else:
                assert (brute["count"] >= 2).mean() > 0.3, case
            tmax, after = key_mix(brute, 3)
            same(s.multihit_host(org, d, 3, tmax, after, use_bvh=True), s.multihit_host(org, d, 3, tmax, after), f"{case} tmax and key mix")
    s.close()


# the host walk on the mixed scene under SAH, rays_at_triangles(sd, 2048, 13): (rays whose list is not the brute force's first k, hits
# dropped on them) per run — every one an ill-conditioned hit culled behind the bound or tmax (the sliver limit)
MIXED_SAH_LOST = {"k=8": (0, 0), "k=1": (0, 0), "k=4, tmax and key mix": (1, 1), "k=8, tmax on the third hit": (2, 2)}


def test_pre_split_triangles_are_listed_once(devlib):
    """closest_scenes.mixed_scene() under SAH: the two scene-spanning triangles are pre-split and sit whole in many leaves. On all 2,048
    rays the walk is held to the contract with its stated limit (multihit_scenes.held_to_the_limit): its list is the brute force's with
    nothing but ill-conditioned hits dropped — the brute force's list itself on every ray without such a hit, 1,822 of them. The rays on
    which the walk does drop one are counted and the counts asserted (they are DESIGN.md §24's). The two spanning triangles appear in some
    lists and never twice in one; and the model over the LEAF RECORDS with the de-duplication left out lists a triangle twice — so a
    kernel without it could not pass."""
    import closest_scenes as cs
    sd, mask = cs.mixed_scene()
    s = Scene(sd, -1, abi.RT_BVH_SAH, lib=devlib)
    assert s.info().n_split_triangles > 0
    s.check_bvh()
    org, d = ms.rays_at_triangles(sd, 2048, 13)
    ok = ms.well_conditioned(s, org, d)
    assert ok.sum() == 1822  # the other 226 have a hit on a sliver whose fp32 t is not its true t: the limit's ground
    brute = s.multihit_host(org, d, 8)
    assert (brute["count"] >= 2).mean() > 0.5
    walk = s.multihit_host(org, d, 8, use_bvh=True)
    same({k: a[ok] for k, a in walk.items() if k in ms.OUTPUTS}, {k: a[ok] for k, a in brute.items() if k in ms.OUTPUTS}, "mixed sah k=8")
    tmax, after = key_mix(brute, 9)
    t3 = np.where(brute["count"] >= 3, brute["t"][:, 2], f32(np.inf)).astype(f32)
    lost = {}
    for what, k, tm, key in (("k=8", 8, None, None), ("k=1", 1, None, None), ("k=4, tmax and key mix", 4, tmax, after), ("k=8, tmax on the third hit", 8, t3, None)):
        got = s.multihit_host(org, d, k, tm, key, use_bvh=True)
        lost[what] = ms.held_to_the_limit(got, s, org, d, k, tm, key, f"mixed sah, {what}")
    print(f"mixed scene, 2,048 rays, {(~ok).sum()} with an ill-conditioned hit; (rays whose list differs, hits dropped): {lost}")
    assert lost == MIXED_SAH_LOST
    org, d = np.ascontiguousarray(org[ok]), np.ascontiguousarray(d[ok])
    walk = {k: a[ok] for k, a in walk.items() if k in ms.OUTPUTS}
    wv = ms.world_tris(sd)
    span = np.flatnonzero((np.abs(wv) == 1).all((1, 2)))  # closest_scenes.mixed_vertices: corners of the cube [-1, 1]^3
    assert len(span) == 2
    gi = s.tree()["global_index"]
    assert all((gi == j).sum() > 1 for j in span)  # in several leaves
    for j in span:
        in_list = (walk["tri"] == j).sum(1)
        assert in_list.max() == 1 and in_list.sum() > 50, j
    # every list: no index twice
    srt = np.sort(walk["tri"], 1)
    assert not ((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] != NO_TRI)).any()
    # the table over the records of the rays that hit a spanning triangle, the duplicates left in
    rays = np.flatnonzero((walk["tri"][:, :4] == span[0]).any(1) | (walk["tri"][:, :4] == span[1]).any(1))[:64]
    assert len(rays) == 64
    tab = ms.oracle_table(wv[span], org[rays], d[rays])
    rows = np.concatenate([np.repeat(i, (gi == j).sum()) for i, j in enumerate(span)])
    recs = {k: a[rows] for k, a in tab.items()}
    with_dups = multihit_model(recs, 8, index=span[rows])
    once = multihit_model(tab, 8, index=span)
    assert (once["count"] >= 1).all() and not np.array_equal(with_dups["tri"], once["tri"])
    assert (with_dups["tri"][:, 0] == with_dups["tri"][:, 1]).all()
    s.close()


def test_the_moving_bound_visits_fewer_nodes_on_the_full_pile(devlib):
    """The pile of 8,192 parallel triangles, 256 aimed rays: the walk with k = 8 visits fewer nodes and tests fewer triangles than the same
    walk with a list that never fills (k = the triangle count: the bound stays at tmax), and both equal the brute force's counts."""
    import closest_scenes as cs
    sd = cs.pile_scene()
    s = Scene(sd, -1, abi.RT_BVH_SAH, lib=devlib)
    assert s.tree()["stack_need"] > cs.K_LDS_STACK
    org, d = aimed_rays(sd, 256, 7)
    brute = s.multihit_host(org, d, 8)
    moving = s.multihit_host(org, d, 8, use_bvh=True)
    held = s.multihit_host(org, d, 8192, use_bvh=True, slots=False)
    same(moving, brute, "pile k=8")
    np.testing.assert_array_equal(np.minimum(held["count"], 8), brute["count"])
    assert (held["count"] > 8).mean() > 0.4 and held["count"].max() > 1000
    print(f"pile, 256 rays: k = 8 {moving['node_visits']} node visits, {moving['tri_tests']} triangle tests; "
          f"bound held at tmax {held['node_visits']} and {held['tri_tests']}")
    assert moving["node_visits"] < held["node_visits"] and moving["tri_tests"] < held["tri_tests"]
    s.close()


# ---- above the ABI -------------------------------------------------------------------------------------------------------------------------
def test_trace_all_crossings_and_inside_mask_on_the_cube(rtlib):
    """The cube, closed: points inside and outside along one oblique direction. Chosen so that the oracle's table shows no two hits at
    equal t on any ray (no ray meets an edge or a vertex): inside points cross once, outside points twice or not at all."""
    sd = scenes.get_scene("cube")
    wv = ms.world_tris(sd)
    lo, hi = wv.reshape(-1, 3).min(0), wv.reshape(-1, 3).max(0)
    g = np.random.default_rng(2)
    inside = g.uniform(lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo), (300, 3))
    outside = g.uniform(lo - 1.0 * (hi - lo), hi + 1.0 * (hi - lo), (600, 3))
    outside = outside[((outside < lo) | (outside > hi)).any(1)]
    pts = np.ascontiguousarray(np.concatenate([inside, outside]), f32)
    direction = np.array([0.31, 0.52, 0.79], f32)
    dirs = np.ascontiguousarray(np.broadcast_to(direction, pts.shape))
    tab = ms.oracle_table(wv, pts, dirs)
    cnt = counting(tab)
    ts = np.sort(np.where(cnt, tab["t"], np.inf), 0)
    assert not ((ts[1:] == ts[:-1]) & np.isfinite(ts[1:])).any()  # no equal-t pair on any ray
    s = Scene(sd, device=-1)
    off, t, u, v, tri = s.trace_all(pts, dirs, page=1)
    want = multihit_model(tab, 12)
    np.testing.assert_array_equal(np.diff(off), want["count"])
    filled = np.arange(12)[None, :] < want["count"][:, None]
    np.testing.assert_array_equal(t, want["t"][filled])
    np.testing.assert_array_equal(tri, want["tri"][filled])
    assert off.dtype == np.int64 and t.dtype == f32 and tri.dtype == np.uint32
    x = bake.crossings(s, pts, dirs)
    np.testing.assert_array_equal(x, want["count"])
    assert (x[:300] == 1).all() and np.isin(x[300:], (0, 2)).all() and (x[300:] == 2).any() and (x[300:] == 0).any()
    mask = bake.inside_mask(s, pts, direction)
    assert mask.dtype == bool and mask[:300].all() and not mask[300:].any()
    short = bake.crossings(s, pts, dirs, np.full(len(pts), 1e-3, f32))
    assert (short <= x).all() and (short < x).any()
    assert "closed" in bake.inside_mask.__doc__ and "edge" in bake.inside_mask.__doc__ and "vertex" in bake.inside_mask.__doc__
    s.close()


# ---- what the unit relies on in texts it does not own --------------------------------------------------------------------------------------
def test_what_the_kernel_relies_on_in_the_traversal(devlib):
    """rt_multihit.hip opens a ray's list at the step that finds cur == 0 and carries k and the key to it in T.best.u / v / tri. That holds
    while (1) trav_begin is the only text of rt_device.h that sets cur to the root, (2) no node has the root as a child, so no push, descent
    or pop brings cur back to 0, and (3) trav_inner reads nothing of T.best but best.t and writes none of it. rt_device.h is not this
    unit's to annotate (the render kernels' listings depend on it), so the three are held here; an edit that breaks one fails this test
    and not, silently, the lists."""
    src = (REPO / "sycl-ray-tracer_amd" / "csrc" / "rt_device.h").read_text()
    body = lambda name: re.search(rf"^RT_DEV void {name}\(.*?^}}", src, re.M | re.S).group(0)
    assert len(re.findall(r"\bcur = 0;", src)) == 1 and "T.cur = 0;" in body("trav_begin")
    inner = re.sub(r"//.*", "", body("trav_inner"))
    assert set(re.findall(r"\bbest\.\w+", inner)) == {"best.t"} and not re.search(r"\bbest\.t\s*=[^=]", inner) and "T.best" in inner
    assert not re.search(r"[(,]\s*T\.best\s*[,)]", inner)  # nor handed on whole
    import closest_scenes as cs
    from test_scene_update import chain_scene
    for sd, builder in ((cs.mixed_scene()[0], abi.RT_BVH_SAH), (scenes.get_scene("cornell"), abi.RT_BVH_LBVH), (chain_scene(), abi.RT_BVH_LBVH)):
        s = Scene(sd, -1, builder, lib=devlib)
        nodes = s.tree()["nodes"]
        assert len(nodes) > 1 and (nodes[:, 12:16].view(np.int32) != 0).all()  # child words: >= 0 an inner node's index, and never the root's
        s.close()


# ---- the listing ---------------------------------------------------------------------------------------------------------------------------
def _k_multihit(n):
    return f"_ZN2rt10k_multihitILj{n}EEEvNS_8SceneDevENS_8MultiDevE"


def test_multihit_kernels_have_the_resources_design_states_and_pass_the_hazard_scan(tmp_path):
    """k_multihit<2>, <4>, <8> (rt_multihit.hip): registers, spills, scratch, LDS and occupancy are the figures of DESIGN.md §24, read from
    the listing and from DESIGN.md itself. No VGPR is spilled and the scratch is exactly the frame every RT_TRAVERSAL_LDS kernel has
    (k_query's: the traversal stack's spill array): the lists live in registers. The unit carries the asm node fetch (trav_inner) and
    passes tests/test_isa_hazards.py's checker."""
    from test_denoise import _listing
    from test_isa_hazards import _check
    from test_svgf import _metadata
    lines = _listing("rt_multihit.hip", tmp_path)
    meta = "\n".join(lines)
    groups = _check(lines)
    design = (REPO / "DESIGN.md").read_text()
    kq = _metadata("\n".join(_listing("rt_query.hip", tmp_path)), "_ZN2rt7k_queryILb0EEEvNS_8SceneDevENS_8QueryDevE", "private_segment_fixed_size")
    assert kq == 224
    names = re.findall(r"^(_ZN2rt10k_multihitILj\dE\S+):", meta, re.M)
    occs = [int(x) for x in re.findall(r"^; Occupancy: (\d+)", meta, re.M)]
    assert len(names) == 3 and len(occs) == 3  # three kernels in the unit, in the listing's order
    occ = dict(zip(names, occs))
    for n in (2, 4, 8):
        sym = _k_multihit(n)
        assert any(f"k_multihitILj{n}E" in k for k in groups), groups
        got = {k: _metadata(meta, sym, k) for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size",
                                                    "group_segment_fixed_size")}
        got["occupancy"] = occ[sym]
        m = re.search(rf"`k_multihit<{n}>`: (\d+) VGPRs, (\d+) SGPRs, (\d+) VGPRs spilled, (\d+) bytes of scratch per lane, ([\d,]+) bytes of LDS "
                      r"per workgroup, (\d+) waves per SIMD", design)
        assert m, f"DESIGN.md states k_multihit<{n}>'s resources in one sentence"
        stated = {"vgpr_count": int(m.group(1)), "sgpr_count": int(m.group(2)), "vgpr_spill_count": int(m.group(3)),
                  "private_segment_fixed_size": int(m.group(4)), "group_segment_fixed_size": int(m.group(5).replace(",", "")),
                  "occupancy": int(m.group(6))}
        assert got == stated, n
        assert got["vgpr_spill_count"] == 0 and got["private_segment_fixed_size"] == kq
        assert got["vgpr_count"] * got["occupancy"] <= 512 and (got["occupancy"] // 2) * got["group_segment_fixed_size"] <= 160 * 1024
    # the only scratch instructions are the spill array's, addressed by the entry's register, never a spill slot's constant offset
    scratch = [ln.strip() for ln in lines if re.match(r"\s+scratch_", ln)]
    assert scratch and all(re.fullmatch(r"scratch_(load|store)_dword v\d+, v\d+, off", ln) for ln in scratch), scratch
    src = (REPO / "sycl-ray-tracer_amd" / "csrc" / "rt_multihit.hip").read_text()
    assert "tri_test_regs(" in src and "trav_inner(" in src and "query_frame<" in src and "asm" not in src  # nothing of the traversal restated
    # the list's store and the whole-leaf read have one text each (rt_hit_list.h, rt_whole_leaf.h), no second one in a unit
    csrc = REPO / "sycl-ray-tracer_amd" / "csrc"
    for unit in ("rt_multihit.hip", "rt_nearest.hip"):
        assert "store_slot" not in (csrc / unit).read_text(), unit
    for unit in ("rt_multihit.hip", "rt_nearest.hip", "rt_closest.hip"):
        assert "tri_ld4(" not in (csrc / unit).read_text(), unit
