"""The origin skip without a GPU (csrc/rt_types.h: SkipRec): the table the host builder makes — one entry per triangle naming
the highest ancestor proven flat on the triangle's plane — passes rt_scene_check_bvh on every kind of scene, the checker catches an entry
that names a subtree it cannot prove, the scenes that must not skip hold nothing but the no-match word, and the host walk with the skip
(rt_scene_count_visits mode 4, the kernels' own fp32 test) finds exactly the hits of the walk without it."""
import ctypes as C

import numpy as np
import pytest

from rtamd import abi, scenes

NONE = 0xFFFFFFFF
SKIP_NONE = 1  # kSkipNone

SCENES = {
    "atrium": lambda: scenes.atrium_scene(1),
    "cube": scenes.cube_scene,
    "cornell": scenes.cornell_scene,
    "voxel": lambda: scenes.voxel_scene(1),
    "atrium_tilted": lambda: scenes.atrium_tilted_scene(1, coarse=True),
    "atrium_rotated": lambda: scenes.atrium_tilted_scene(1, coarse=False),
}


@pytest.fixture(scope="module")
def built(devlib):
    """every scene once, host only, by the developer library (which can show and overwrite the table): name -> (desc, handle)"""
    out = {}
    for name, make in SCENES.items():
        sd = make()
        c = sd.to_c()
        h = C.c_void_p()
        abi.check(devlib.rt_scene_create(C.byref(c), -1, abi.RT_BVH_SAH, C.byref(h)), devlib)
        out[name] = (sd, h)
    yield out
    for _sd, h in out.values():
        devlib.rt_scene_destroy(h)


def _table(devlib, h):
    n = C.c_uint32(0)
    abi.check(devlib.rt_dev_scene_skip_table(h, C.byref(n), None, 0, 0), devlib)
    words = np.zeros((n.value, 8), np.uint32)
    abi.check(devlib.rt_dev_scene_skip_table(h, C.byref(n), abi.u32ptr(words), n.value, 0), devlib)
    return words


def _write(devlib, h, words):
    n = C.c_uint32(0)
    abi.check(devlib.rt_dev_scene_skip_table(h, C.byref(n), abi.u32ptr(np.ascontiguousarray(words)), words.shape[0], 1), devlib)


@pytest.mark.parametrize("name", list(SCENES))
def test_the_table_passes_the_checker_and_names_subtrees_where_walls_are_flat(devlib, built, name):
    sd, h = built[name]
    abi.check(devlib.rt_scene_check_bvh(h), devlib)
    words = _table(devlib, h)
    assert words.shape[0] == sd.n_triangles
    named = words[:, 0] != SKIP_NONE
    # a word is a node's byte offset or a leaf code, never anything else
    w = words[named, 0]
    assert np.all(((w & 0x80000000) != 0) | (w % 64 == 0))
    n = words[named, 1:4].view(np.float32).astype(np.float64)
    np.testing.assert_allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-6)
    # the entries' normals are the triangles' own, either way round
    tw = sd.world_triangles()[named]
    g = np.cross(tw[:, 1] - tw[:, 0], tw[:, 2] - tw[:, 0])
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    assert np.all(np.abs(np.sum(g * n, 1)) > 1 - 1e-5)
    share = float(named.mean())
    print(f"{name}: {sd.n_triangles} triangles, {100 * share:.1f} % with a subtree to skip")
    if name in ("atrium", "cornell", "voxel", "atrium_tilted", "atrium_rotated"):
        assert share > 0.3, "flat walls, axis-aligned or rotated, must be found"


def _parents(devlib, h):
    """the host tree: nodes (n, 16) as int32 words, leaf record -> global index"""
    sc = [C.c_uint32(0) for _ in range(4)]
    bb, pad, bounds = C.c_int32(0), C.c_float(0), (C.c_float * 6)()
    args = [C.byref(sc[0]), C.byref(sc[1]), C.byref(sc[2]), C.byref(sc[3]), C.byref(bb), C.byref(pad), bounds]
    abi.check(devlib.rt_dev_scene_tree(h, *args, None, None, None, 0), devlib)
    cap = max(sc[0].value, sc[1].value, sc[2].value)
    nodes = np.zeros((cap, 16), np.int32)
    gidx = np.zeros(cap, np.uint32)
    wv = np.zeros(cap, np.float32)
    abi.check(devlib.rt_dev_scene_tree(h, *args, nodes.ctypes.data_as(C.c_void_p), abi.u32ptr(gidx), abi.fptr(wv), cap), devlib)
    nodes = nodes[: sc[0].value]
    parent = {}
    for i in range(nodes.shape[0]):
        for k in range(4):
            c = int(nodes[i, 12 + k])
            if c >= 0:
                parent[c] = i
    return nodes, parent


def test_the_checker_catches_entries_it_cannot_prove(devlib, built):
    sd, h = built["atrium"]
    good = _table(devlib, h)
    nodes, parent = _parents(devlib, h)
    named = np.flatnonzero((good[:, 0] != SKIP_NONE) & ((good[:, 0] & 0x80000000) == 0))
    assert named.size
    caught = 0

    def refused(words, what):
        _write(devlib, h, words)
        rc = devlib.rt_scene_check_bvh(h)
        msg = devlib.rt_last_error().decode()
        _write(devlib, h, good)
        assert rc == abi.RT_ERR_INVALID and "origin-skip" in msg, f"{what}: {rc} {msg}"
        return msg

    # one level further up than the builder went: a subtree that is not coplanar with the triangle (or too large to prove)
    for t in named[:: max(1, named.size // 40)]:
        node = int(good[t, 0]) // 64
        if parent.get(node, 0) == 0:
            continue
        bad = good.copy()
        bad[t, 0] = parent[node] * 64
        msg = refused(bad, "the parent of the highest proven ancestor")
        assert "not coplanar" in msg or "names no subtree" in msg
        caught += 1
    assert caught >= 10
    t = int(named[0])
    # another triangle's subtree
    other = next(int(u) for u in named if good[u, 0] != good[t, 0] and abs(float(np.dot(good[u, 1:4].view(np.float32), good[t, 1:4].view(np.float32)))) < 0.5)
    bad = good.copy()
    bad[t, 0] = good[other, 0]
    assert "not in the subtree" in refused(bad, "a subtree the triangle is not in")
    # the right subtree with another plane, with thresholds below the proof's, with a word that is no child word
    bad = good.copy()
    bad[t, 1:4] = good[other, 1:4]
    assert "not coplanar" in refused(bad, "another triangle's normal")
    bad = good.copy()
    bad[t, 7] = 0
    assert "thresholds" in refused(bad, "thresholds of zero")
    bad = good.copy()
    bad[t, 0] = 0
    assert "not a child word" in refused(bad, "the root")
    bad = good.copy()
    bad[t, 4] ^= 0x00400000
    assert "first vertex" in refused(bad, "a point off the triangle")
    abi.check(devlib.rt_scene_check_bvh(h), devlib)


def test_scenes_that_must_not_skip_hold_only_the_no_match_word(devlib):
    sd = scenes.cornell_scene()
    c = sd.to_c()
    h = C.c_void_p()
    abi.check(devlib.rt_scene_create_ex(C.byref(c), -1, abi.RT_BVH_SAH, abi.RT_SCENE_UPDATABLE, C.byref(h)), devlib)
    words = _table(devlib, h)
    assert words.shape[0] == sd.n_triangles and np.all(words[:, 0] == SKIP_NONE)
    abi.check(devlib.rt_scene_check_bvh(h), devlib)
    devlib.rt_scene_destroy(h)
    # a scene 10^4 across: the fp32 rounding of origin - p alone is worth more than kTNear / 4 on a wall that size
    big = sd.updated(positions=sd.positions * np.float32(1e4))
    c = big.to_c()
    abi.check(devlib.rt_scene_create(C.byref(c), -1, abi.RT_BVH_SAH, C.byref(h)), devlib)
    words = _table(devlib, h)
    assert words.shape[0] == sd.n_triangles and np.all(words[:, 0] == SKIP_NONE)
    abi.check(devlib.rt_scene_check_bvh(h), devlib)
    devlib.rt_scene_destroy(h)
    # the same scene at its own size does skip
    c = sd.to_c()
    abi.check(devlib.rt_scene_create(C.byref(c), -1, abi.RT_BVH_SAH, C.byref(h)), devlib)
    walls = np.flatnonzero(sd.tri_instance < 5)
    assert np.all(_table(devlib, h)[walls, 0] != SKIP_NONE)
    devlib.rt_scene_destroy(h)


def _camera_rays(lib, sd, w, h):
    cam = abi.rt_camera()
    ce = (C.c_float * 3)(*[float(v) for v in sd.camera.position])
    di = (C.c_float * 3)(*[float(v) for v in sd.camera.direction])
    abi.check(lib.rt_camera_init(C.byref(cam), w, h, ce, di, float(sd.camera.focal_length)), lib)
    p00, du, dv, c0 = (np.array(list(getattr(cam, k)), np.float32) for k in ("pixel00", "delta_u", "delta_v", "center"))
    ys, xs = np.mgrid[0:h, 0:w]
    d = p00 + xs[..., None].astype(np.float32) * du + ys[..., None].astype(np.float32) * dv - c0
    return np.broadcast_to(c0, (h * w, 3)).copy(), d.reshape(-1, 3).astype(np.float32)


def _walk(lib, h, org, dirs, mode, start=None):
    n = org.shape[0]
    org, dirs = np.ascontiguousarray(org, np.float32), np.ascontiguousarray(dirs, np.float32)
    v, tt = C.c_uint64(0), C.c_uint64(0)
    t = np.zeros(n, np.float32)
    tri = np.full(n, NONE, np.uint32) if start is None else np.ascontiguousarray(start, np.uint32).copy()
    abi.check(lib.rt_scene_count_visits(h, n, abi.fptr(org), abi.fptr(dirs), mode, C.byref(v), C.byref(tt), abi.fptr(t), abi.u32ptr(tri)), lib)
    return v.value, tt.value, t, tri


def _leave(n, d, rng):
    """directions that leave a surface with normal n (facing the incoming direction d): mirror reflections, rays INTO the surface (what a
    dielectric refracts), rays nearly along it, diffuse continuations — through half storage, as the kernels keep them"""
    u = rng.uniform(-1, 1, size=n.shape)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    kind = rng.integers(0, 4, size=n.shape[0])[:, None]
    dn = d / (np.linalg.norm(d, axis=1, keepdims=True) + 1e-30)
    out = np.where(kind == 0, dn - 2 * np.sum(dn * n, 1, keepdims=True) * n,
                   np.where(kind == 1, dn + 0.2 * u,
                            np.where(kind == 2, n * 1e-3 + u - np.sum(u * n, 1, keepdims=True) * n, n + u)))
    return out.astype(np.float16).astype(np.float32)


def _facing(tw, tri, d):
    w = tw[tri]
    n = np.cross(w[:, 1] - w[:, 0], w[:, 2] - w[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True) + 1e-30
    return np.where((np.sum(n * d, 1) > 0)[:, None], -n, n)


@pytest.mark.parametrize("name", list(SCENES))
def test_the_host_walk_with_the_skip_finds_the_hits_of_the_walk_without(devlib, built, name):
    """At least 100 k rays per scene that start on a surface, as the renderers make them (fp32 origin + direction * t, the direction through
    half storage): generations of a camera-ray chain, and — where the chain dies out before 100 k, as on the cube, which stands in the
    open — rays that arrive at points spread over the scene's triangles by area."""
    sd, h = built[name]
    tw = sd.world_triangles()
    rng = np.random.default_rng(11)
    org, dirs = _camera_rays(devlib, sd, 352, 198)
    _, _, t, tri = _walk(devlib, h, org, dirs, 0)
    total = visits0 = visits4 = tests0 = tests4 = 0

    def both(org, dirs, start):
        nonlocal total, visits0, visits4, tests0, tests4
        v0, t0, t, tri = _walk(devlib, h, org, dirs, 0)
        v4, t4, ts, tris = _walk(devlib, h, org, dirs, 4, start)
        np.testing.assert_array_equal(tris, tri)
        np.testing.assert_array_equal(ts, t)
        assert v4 <= v0 and t4 <= t0
        total += org.shape[0]
        visits0, visits4, tests0, tests4 = visits0 + v0, visits4 + v4, tests0 + t0, tests4 + t4
        return t, tri

    for gen in range(8):
        hit = tri != NONE
        if not hit.any() or total >= 100_000:
            break
        d = dirs[hit]
        start = tri[hit]
        out = _leave(_facing(tw, start, d), d, rng)
        org = (org[hit] + (d * t[hit][:, None]).astype(np.float32)).astype(np.float32)
        dirs = out
        t, tri = both(org, dirs, start)
    chain = total
    if total < 100_000:  # rays that arrive at points of the triangles themselves: from a point 0.5 .. 3 scene scales away, origin + direction * t in fp32
        m = 100_000 - total
        area = 0.5 * np.linalg.norm(np.cross(tw[:, 1] - tw[:, 0], tw[:, 2] - tw[:, 0]), axis=1)
        start = rng.choice(tw.shape[0], size=m, p=area / area.sum()).astype(np.uint32)
        b = rng.uniform(0, 1, size=(m, 2))
        b = np.where((b.sum(1) > 1)[:, None], 1 - b, b)
        w = tw[start]
        x = w[:, 0] + b[:, :1] * (w[:, 1] - w[:, 0]) + b[:, 1:] * (w[:, 2] - w[:, 0])
        d = rng.uniform(-1, 1, size=(m, 3))
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        scale = float(np.ptp(tw.reshape(-1, 3), axis=0).max())
        tt = rng.uniform(0.5, 3.0, size=(m, 1)).astype(np.float32) * np.float32(scale)
        far = (x - d.astype(np.float64) * tt).astype(np.float32)
        org = (far + (d * tt).astype(np.float32)).astype(np.float32)
        dirs = _leave(_facing(tw, start, d), d, rng)
        both(org, dirs, start)
    print(f"{name}: {total} surface rays ({chain} of a camera chain), node visits {visits0 / total:.2f} -> {visits4 / total:.2f}, triangle tests {tests0 / total:.2f} -> {tests4 / total:.2f}")
    assert total >= 100_000
    if name in ("atrium", "cornell", "atrium_rotated", "cube"):  # (a quarter of these rays graze their surface and may not skip; the rest must)
        assert tests4 < 0.9 * tests0, "the skip must take effect"
    # mode 4 needs the start triangles, in range
    assert devlib.rt_scene_count_visits(h, 1, abi.fptr(org), abi.fptr(dirs), 4, None, None, None, None) == abi.RT_ERR_INVALID
    bad = np.array([sd.n_triangles], np.uint32)
    assert devlib.rt_scene_count_visits(h, 1, abi.fptr(org), abi.fptr(dirs), 4, None, None, None, abi.u32ptr(bad)) == abi.RT_ERR_INVALID
