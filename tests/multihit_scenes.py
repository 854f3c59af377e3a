"""What the multi-hit tests share (tests/test_multihit.py: the host statement; tests/test_gpu_multihit.py: the device): the expected value
of every comparison, built from the CPU oracle ALONE, and the rays.

The oracle's brute force on a scene of ONE triangle is that triangle's own candidate for a ray — mt_hit's (t, u, v), or a miss. A table of
such runs over every triangle of a scene, sorted per ray by (t, index), is every counting hit of every ray in the contract's order
(include/rt_mi355x.h: rt_multihit_query). A plain module; everything is seeded, built once per process and never changed."""
import numpy as np

from rtamd import scenes
from test_closest_points import NO_TRI, bounds_of, tri_scene

f32 = np.float32
OUTPUTS = ("t", "u", "v", "tri", "count")
_tables = {}


def oracle_table(wverts, org, dirs, key=None):
    """-> {"t", "u", "v": (T, n) float32, "hit": (T, n) bool}: OracleScene.intersect(org, dirs, False) on tri_scene([w_j]) for every
    triangle j of wverts (T, 3, 3). `key`: a name to cache the table under (the caller's scene and ray set)."""
    from oracle import oracle as O
    if key is not None and key in _tables:
        return _tables[key]
    wverts = np.asarray(wverts, f32).reshape(-1, 3, 3)
    org, dirs = np.ascontiguousarray(org, f32), np.ascontiguousarray(dirs, f32)
    T, n = len(wverts), len(org)
    tab = {"t": np.zeros((T, n), f32), "u": np.zeros((T, n), f32), "v": np.zeros((T, n), f32), "hit": np.zeros((T, n), bool)}
    for j in range(T):
        osc = O.OracleScene(tri_scene("one", wverts[j:j + 1]))
        t, u, v, tri = osc.intersect(org, dirs, False)
        tab["t"][j], tab["u"][j], tab["v"][j], tab["hit"][j] = t, u, v, tri != NO_TRI
        assert ((tri == 0) | (tri == NO_TRI)).all()
    for a in tab.values():
        a.setflags(write=False)
    if key is not None:
        _tables[key] = tab
    return tab


def counting(table, tmax=None, after=None, index=None):
    """(T, n) bool: the candidates that count — a hit, t <= tmax, (t, index) > (after_t, after_tri). NaN tmax or key: nothing."""
    t = table["t"]
    idx = (np.arange(t.shape[0], dtype=np.uint32) if index is None else np.asarray(index, np.uint32))[:, None]
    ok = table["hit"].copy()
    if tmax is not None:
        ok &= t <= np.asarray(tmax, f32)[None, :]
    if after is not None:
        at, atri = np.asarray(after[0], f32)[None, :], np.asarray(after[1], np.uint32)[None, :]
        ok &= (t > at) | ((t == at) & (idx > atri))
    return ok


def multihit_model(table, k, tmax=None, after=None, index=None):
    """The contract in numpy: filter, stable sort by (t, index), first k. `index` (T,): the triangle index of every table row (default: the
    row) — a table with a triangle's row repeated and no de-duplication lists that triangle twice: what the kernel must NOT do.
    -> {"t", "u", "v": (n, k) float32, "tri": (n, k) uint32, "count": (n,) uint32}"""
    t = table["t"]
    T, n = t.shape
    idx = np.arange(T, dtype=np.uint32) if index is None else np.asarray(index, np.uint32)
    ok = counting(table, tmax, after, idx)
    order = np.lexsort((np.broadcast_to(idx[:, None], (T, n)), t, ~ok), axis=0)[:k]  # counting first, then t, then index
    kk = order.shape[0]
    cols = np.arange(n)[None, :]
    filled = ok[order, cols]
    out = {"t": np.full((n, k), np.inf, f32), "u": np.zeros((n, k), f32), "v": np.zeros((n, k), f32), "tri": np.full((n, k), NO_TRI, np.uint32)}
    for name in ("t", "u", "v"):
        out[name][:, :kk] = np.where(filled, table[name][order, cols], out[name][:, :kk].T).T
    out["tri"][:, :kk] = np.where(filled, np.broadcast_to(idx[:, None], (T, n))[order, cols], np.uint32(NO_TRI)).T
    out["count"] = filled.sum(0).astype(np.uint32)
    return out


def hits_per_ray(table, tmax=None, after=None):
    return counting(table, tmax, after).sum(0)


def aimed_rays(sd, n, seed):
    """Rays that cross the scene: the origin two scene diagonals out from a uniform point inside the bounds, along a random direction; the
    direction unnormalised, its length uniform in 0.5 .. 2. -> (org, dirs) (n, 3) float32"""
    g = np.random.default_rng(seed)
    lo, hi, _ = bounds_of(sd)
    p = g.uniform(lo, hi, (n, 3))
    w = g.normal(size=(n, 3))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    diag = np.linalg.norm(hi - lo)
    org = p - 2.0 * diag * w
    return np.ascontiguousarray(org, f32), np.ascontiguousarray(w * g.uniform(0.5, 2.0, (n, 1)), f32)


def rays_at_triangles(sd, n, seed):
    """aimed_rays whose directions go through the centroid of a random triangle each (fp64, then rounded): on a scene of tiny triangles in
    much empty space a ray through a uniform point meets nothing but the large ones"""
    g = np.random.default_rng(seed)
    org, dirs = aimed_rays(sd, n, seed)
    cen = world_tris(sd).astype(np.float64).mean(1)
    c = cen[g.integers(0, len(cen), n)]
    return org, np.ascontiguousarray((c - org) * g.uniform(0.5, 2.0, (n, 1)), f32)


K_ALL = 64  # slots that hold EVERY counting hit of a ray on the mixed scene (asserted where used)


def ill_conditioned(scene, org, dirs, hits):
    """(n, k) bool: the filled slots of `hits` (a multihit_host result: the brute force's) whose fp32 t is more than pad / 2 along the ray from
    the t of the same test in float64 on the same fp32 vertices, pad = 2e-5 x scene scale being the builder's padding. A child box is kept
    iff the ray enters it in front of the bound; it holds its triangles' true surface with at least half that padding to spare
    (rt_scene_check_bvh). The candidate's t is the fp32 test's, though, and on a sliver that is not the true t: the mixed scene has hits
    whose fp32 t is 0.6 % off (det ~ 1e-5), far outside the box. Behind a bound (the k-th entry, or tmax) between the two the box is culled
    and the brute force still lists the hit — for the closest hit of rt_intersect_batch and rt_trace_rays as much as here. The contract
    states this limit (include/rt_mi355x.h: rt_multihit_query). Geometry and the reference alone decide which hits these
    are; nothing of the walk or the kernel is looked at. (A NaN or infinite float64 t — a degenerate triangle the fp32 test let through —
    is ill-conditioned.)"""
    sd = scene.desc
    wv = world_tris(sd).astype(np.float64)
    _, _, scale = bounds_of(sd)
    pad = 2e-5 * float(scale)
    ray, slot = np.nonzero(hits["tri"] != NO_TRI)
    tri = hits["tri"][ray, slot]
    o, d = org.astype(np.float64)[ray], dirs.astype(np.float64)[ray]
    v0 = wv[tri, 0]
    e1, e2 = wv[tri, 1] - v0, wv[tri, 2] - v0
    q = np.cross(o - v0, e1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t64 = (e2 * q).sum(1) / (e1 * np.cross(d, e2)).sum(1)
        off = np.abs(hits["t"][ray, slot].astype(np.float64) - t64) * np.linalg.norm(d, axis=1)
    bad = np.zeros(hits["tri"].shape, bool)
    bad[ray, slot] = ~(off <= 0.5 * pad)
    return bad


def well_conditioned(scene, org, dirs):
    """(n,) bool: the rays none of whose counting hits (the brute force's, all of them) is ill_conditioned: there a list IS the brute force's"""
    all_hits = scene.multihit_host(org, dirs, K_ALL)
    assert (all_hits["count"] < K_ALL).all()
    return ~ill_conditioned(scene, org, dirs, all_hits).any(1)


def _equal(a, b):
    """elementwise, as assert_array_equal compares: equal values, or NaN in both"""
    return (a == b) | ((a != a) & (b != b))


def held_to_the_limit(got, scene, org, dirs, k, tmax=None, after=None, what=""):
    """The contract on EVERY ray, its stated limit included: `got` (a walk's or the device's lists of k) against the brute force's list of
    all counting hits under the same tmax and key. A ray's list must be the brute force's with nothing but ill_conditioned hits dropped:
    the filled slots are a subsequence of the brute force's, equal in t, u, v and tri; every brute-force hit skipped in front of a
    listed one is ill-conditioned; a list that is not full (count < k) has skipped every hit behind its last, so those are ill-conditioned
    too; the slots past count hold the miss. On a ray without an ill-conditioned hit that is equality with the brute force's first k.
    -> (rays whose list differs from the brute force's first k, hits dropped on them)"""
    full = scene.multihit_host(org, dirs, K_ALL, tmax, after)
    assert (full["count"] < K_ALL).all(), what
    bad = ill_conditioned(scene, org, dirs, full)
    kk = min(k, K_ALL)
    differs = np.zeros(len(org), bool)
    for name in ("t", "u", "v", "tri"):
        differs |= ~_equal(got[name], full[name][:, :kk]).all(1)
    differs |= got["count"] != np.minimum(full["count"], kk)
    dropped = 0
    for i in np.flatnonzero(differs):
        c, p = int(got["count"][i]), 0
        assert c <= k, (what, i)
        for s in range(c):
            while p < full["count"][i] and full["tri"][i, p] != got["tri"][i, s]:
                assert bad[i, p], f"{what}: ray {i} lost triangle {full['tri'][i, p]} at t = {full['t'][i, p]}, a well-conditioned hit"
                dropped, p = dropped + 1, p + 1
            assert p < full["count"][i], f"{what}: ray {i} lists triangle {got['tri'][i, s]}, which the brute force does not (or not in this order)"
            for name in ("t", "u", "v"):
                assert _equal(got[name][i, s], full[name][i, p]), (what, i, s, name)
            p += 1
        if c < k:
            assert bad[i, p:full["count"][i]].all(), f"{what}: ray {i} ends after {c} of {full['count'][i]} hits, and not all behind are ill-conditioned"
            dropped += int(full["count"][i]) - p
        assert (got["tri"][i, c:] == NO_TRI).all() and np.isposinf(got["t"][i, c:]).all() and not got["u"][i, c:].any() and not got["v"][i, c:].any(), (what, i)
    assert not (differs & ~bad.any(1)).any(), what  # (follows from the above; said once more because it is the point)
    return int(differs.sum()), dropped


def world_tris(sd):
    """the fp32 world vertices as the scene builder computes them, (T, 3, 3)"""
    from rtamd import bake
    return bake.vertex_points(sd)[0]


_cases = {}
N_RAYS, SEED = 2048, 7


def small_case(name):
    """-> dict(sd, wv, org, dirs, table): the Cornell box (116 triangles), closest_scenes.duplicate_scene() (84: seven shuffled cubes) or
    pile_vertices(256), with 2,048 aimed rays of seed 7 and their oracle table. Built once per process."""
    import closest_scenes as cs
    if name not in _cases:
        if name == "cornell":
            sd = scenes.get_scene("cornell")
        elif name == "duplicates":
            sd = cs.duplicate_scene()
        else:
            assert name == "pile256"
            sd = tri_scene("pile256", cs.pile_vertices(256))
        wv = world_tris(sd)
        org, dirs = aimed_rays(sd, N_RAYS, SEED)
        _cases[name] = dict(sd=sd, wv=wv, org=org, dirs=dirs, table=oracle_table(wv, org, dirs, key=name))
    return _cases[name]


def same(got, want, what, names=OUTPUTS):
    for k in names:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")


def tie_straddles(table, k, after=None):
    """(n,) bool: the ray's k-th and (k + 1)-th counting hits have the same t — a tie across slot k - 1"""
    m = multihit_model(table, k + 1, None, after)
    return (m["count"] == k + 1) & (m["t"][:, k - 1] == m["t"][:, k])


def first_hit_key(table):
    """the key (t, tri) of every ray's first counting hit (rays without one: (+inf, 0), nothing counts behind it)"""
    m = multihit_model(table, 1)
    return np.ascontiguousarray(m["t"][:, 0]), np.where(m["count"] == 1, m["tri"][:, 0], 0).astype(np.uint32)


def duplicate_runs(table, k):
    """The runs of a k on the duplicates, [(what, after)]: without a key and with the key of the first hit. The ties are seven-fold, so a
    list of k = 7 without a key ends exactly where a tie group ends; behind the first hit's key the groups are shifted by one and the tie
    straddles slot k - 1 again (and does not for k = 6). Every k from 1 to 8 has a run whose tie straddles on EVERY ray: asserted here."""
    key = first_hit_key(table)
    runs = [("no key", None), ("key on the first hit", key)]
    assert any(tie_straddles(table, k, after).all() for _, after in runs), k
    return runs
