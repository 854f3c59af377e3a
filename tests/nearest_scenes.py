"""What the k-nearest closest-point tests share (tests/test_nearest.py: the host statement; tests/test_gpu_nearest.py: the device): the
expected value of every comparison, built from the numpy model of the closest-point contract ALONE (test_closest_points.closest_candidates),
and the points.

closest_candidates on one triangle is that triangle's candidate (dist2, u, v) for a point. A table of it over every triangle of a scene,
filtered and sorted per point by (dist2, index), is every counting triangle of every point in the contract's order (include/rt_mi355x.h:
rt_nearest_query). A plain module; everything is seeded, built once per process and never changed."""
import numpy as np

import closest_scenes as cs
from rtamd import scenes
from test_closest_points import NO_TRI, bounds_of, closest_candidates, point_mix, tri_scene, world_vertices

f32 = np.float32
OUTPUTS = ("dist2", "u", "v", "tri", "count")
SLOTS = ("dist2", "u", "v", "tri")
_cases = {}


def candidate_table(wverts, pos):
    """-> {"dist2", "u", "v": (T, n) float32}: closest_candidates(pos, v0, v1 - v0, v2 - v0) for every triangle of wverts (T, 3, 3)"""
    wverts = np.asarray(wverts, f32).reshape(-1, 3, 3)
    pos = np.ascontiguousarray(pos, f32)
    T, n = len(wverts), len(pos)
    tab = {"dist2": np.zeros((T, n), f32), "u": np.zeros((T, n), f32), "v": np.zeros((T, n), f32)}
    for j, w in enumerate(wverts):
        tab["dist2"][j], tab["u"][j], tab["v"][j], _ = closest_candidates(pos, w[0][None], (w[1] - w[0])[None], (w[2] - w[0])[None])
    for a in tab.values():
        a.setflags(write=False)
    return tab


def counting(table, max_dist2=None, after=None, index=None):
    """(T, n) bool: the candidates that count — dist2 no NaN, dist2 <= max_dist2, (dist2, index) > (after_dist2, after_tri). A NaN
    max_dist2 or key: nothing."""
    d2 = table["dist2"]
    idx = (np.arange(d2.shape[0], dtype=np.uint32) if index is None else np.asarray(index, np.uint32))[:, None]
    with np.errstate(invalid="ignore"):
        ok = ~np.isnan(d2)
        if max_dist2 is not None:
            ok &= d2 <= np.asarray(max_dist2, f32)[None, :]
        if after is not None:
            ad, atri = np.asarray(after[0], f32)[None, :], np.asarray(after[1], np.uint32)[None, :]
            ok &= (d2 > ad) | ((d2 == ad) & (idx > atri))
    return ok


def nearest_model(table, k, max_dist2=None, after=None, index=None):
    """The contract in numpy: filter, stable sort by (dist2, index), first k. `index` (T,): the triangle index of every table row
    (default: the row) — a table with a triangle's row repeated and no de-duplication lists that triangle twice: what the kernel must NOT
    do. -> {"dist2", "u", "v": (n, k) float32, "tri": (n, k) uint32, "count": (n,) uint32}"""
    d2 = table["dist2"]
    T, n = d2.shape
    idx = np.arange(T, dtype=np.uint32) if index is None else np.asarray(index, np.uint32)
    ok = counting(table, max_dist2, after, idx)
    rows = np.broadcast_to(idx[:, None], (T, n))
    order = np.lexsort((rows, np.where(ok, d2, f32(0)), ~ok), axis=0)[:k]  # counting first, then dist2, then index
    kk = order.shape[0]
    cols = np.arange(n)[None, :]
    filled = ok[order, cols]
    out = {"dist2": np.full((n, k), np.inf, f32), "u": np.zeros((n, k), f32), "v": np.zeros((n, k), f32), "tri": np.full((n, k), NO_TRI, np.uint32)}
    for name in ("dist2", "u", "v"):
        out[name][:, :kk] = np.where(filled, table[name][order, cols], out[name][:, :kk].T).T
    out["tri"][:, :kk] = np.where(filled, rows[order, cols], np.uint32(NO_TRI)).T
    out["count"] = filled.sum(0).astype(np.uint32)
    return out


def same(a, b, what="", keys=OUTPUTS):
    """bit for bit on every output"""
    for k in keys:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k, x.dtype, y.dtype, x.shape, y.shape)
        bad = np.flatnonzero((x.view(np.uint32) != y.view(np.uint32)).reshape(len(x), -1).any(1))
        assert bad.size == 0, f"{what}: {k} differs at {bad.size} entries, first {bad[0]}: {x[bad[0]]} vs {y[bad[0]]}"


def small_case(name):
    """-> dict(sd, pos, wv, table, scale): one of the three small scenes with point_mix(sd, 2048, 7) and its candidate table: the Cornell
    box, seven shuffled cubes (closest_scenes.duplicate_scene) and the first 256 triangles' pile (closest_scenes.pile_vertices(256))."""
    if name in _cases:
        return _cases[name]
    if name == "cornell":
        sd = scenes.get_scene("cornell")
    elif name == "duplicates":
        sd = cs.duplicate_scene()
    else:
        assert name == "pile256"
        sd = tri_scene("pile256", cs.pile_vertices(256))
    pos = point_mix(sd, 2048, 7)
    pos.setflags(write=False)
    wv = world_vertices(sd)
    _cases[name] = dict(sd=sd, pos=pos, wv=wv, table=candidate_table(wv, pos), scale=bounds_of(sd)[2])
    return _cases[name]


def squared_radius(scale, share, n):
    """(n,) float32: the radius share x scale squared in fp32, as Scene.closest_points_multi squares a caller's radius"""
    r = f32(share * scale)
    return np.full(n, r * r, f32)


def within(table, max_dist2=None, after=None):
    return counting(table, max_dist2, after).sum(0)


def first_key(table):
    """the key of every point's first entry: (dist2, tri) of nearest_model(table, 1)"""
    m = nearest_model(table, 1)
    return np.ascontiguousarray(m["dist2"][:, 0]), np.ascontiguousarray(m["tri"][:, 0])


def tie_straddles(table, k, after=None):
    """(n,) bool: slots k - 1 and k of the sorted counting candidates hold equal dist2 — which of the tied triangles stays in a list of k
    is decided by the index alone"""
    m = nearest_model(table, k + 1, None, after)
    return (m["count"] == k + 1) & (m["dist2"][:, k - 1] == m["dist2"][:, k])


def duplicate_runs(table, k):
    """The runs of a k on the duplicates: without a key and behind every point's first entry. On every point a tie straddles slot k - 1
    in one of them at least (asserted in tests/test_nearest.py). -> [(what, after)]"""
    return [("no key", None), ("behind the first entry", first_key(table))]


def key_mix(free, seed):
    """per-point max_dist2 and key around the unbounded answer `free` (k >= 3): closest_scenes.radius_mix around the third entry's dist2
    (on it, the next float below, twice, a tenth, +inf; a few negative, -0.0 and 0); the key on the first entry, one index below it, none
    (-inf) or beyond everything (+inf)"""
    g = np.random.default_rng(seed)
    n = len(free["count"])
    d3 = np.where(free["count"] >= 3, free["dist2"][:, 2], f32(1.0)).astype(f32)
    md2 = cs.radius_mix(d3, seed)
    kk = g.integers(0, 4, n)
    hit = free["count"] >= 1
    d0 = np.where(hit, free["dist2"][:, 0], f32(0.5)).astype(f32)
    j0 = np.where(hit, free["tri"][:, 0], 0).astype(np.uint32)
    ad = np.select([kk == 0, kk == 1, kk == 2], [d0, d0, f32(-np.inf)], f32(np.inf)).astype(f32)
    atri = np.where((kk == 1) & (j0 > 0), j0 - 1, j0).astype(np.uint32)
    return md2, (ad, atri)


def paged(call, pos, page, pages, max_dist2=None):
    """`pages` pages of `page` triangles, EVERY point continued with the key of its last slot: an exhausted point's last slot is the miss,
    (+inf, 0xFFFFFFFF), a key behind which nothing counts, so its later pages stay misses. call(pos, k, max_dist2, after) -> the pages
    side by side, (n, page * pages), and the summed count"""
    out = {k: [] for k in SLOTS}
    count = np.zeros(len(pos), np.uint32)
    key = None
    for _ in range(pages):
        got = call(pos, page, max_dist2, key)
        for k in SLOTS:
            out[k].append(got[k])
        count += got["count"]
        key = (np.ascontiguousarray(got["dist2"][:, page - 1]), np.ascontiguousarray(got["tri"][:, page - 1]))
    res = {k: np.concatenate(v, 1) for k, v in out.items()}
    res["count"] = count
    return res
