"""The origin skip without a GPU (csrc/rt_types.h: SkipRec): the table the host builder makes — one entry per triangle naming
the highest ancestor proven flat on the triangle's plane — passes rt_scene_check_bvh on every kind of scene, the checker catches an entry
that names a subtree it cannot prove, the scenes that must not skip hold nothing but the no-match word, and the host walk with the skip
(rt_scene_count_visits mode 4, the kernels' own fp32 test) finds exactly the hits of the walk without it."""
import ctypes as C

import numpy as np
import pytest

from rtamd import abi, scenes
from rtamd.scenes import CameraPose, Material, SceneBuilder, mesh_box, mesh_cylinder, mesh_quad, trs

NONE = 0xFFFFFFFF
SKIP_NONE = 1  # kSkipNone
K_SKIP_DIST = 40400.0  # kSkipDist
K_SKIP_TILT = 1.0 / 256.0  # kSkipTilt
K_TOP_NODES, K_TOP_SKIP = 341, 309  # kTopNodes; what k_megakernel and k_wf_finish stage of it (RT_TRAVERSAL_LDS_SKIP)


# ---- the scenes the GPU tests render (tests/test_gpu_origin_skip.py imports them) -------------------------------------------------------------
def _room(sb, light=True):
    """a box room of two-triangle walls (each wall's leaf is the whole wall), open to the camera at +z"""
    white = sb.add_material(Material(abi.RT_MAT_DIFFUSE, (0.73, 0.73, 0.73)))
    red = sb.add_material(Material(abi.RT_MAT_DIFFUSE, (0.65, 0.05, 0.05)))
    metal = sb.add_material(Material(abi.RT_MAT_METALLIC, (0.9, 0.85, 0.7), roughness=0.1))
    q = lambda *a, **k: sb.add_mesh(*mesh_quad(*a, **k))
    sb.add_instance(q((-1, -1, 1), (1, -1, 1), (1, -1, -1), (-1, -1, -1)), white)
    sb.add_instance(q((-1, 1, -1), (1, 1, -1), (1, 1, 1), (-1, 1, 1)), white)
    sb.add_instance(q((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1)), metal)
    sb.add_instance(q((-1, -1, 1), (-1, -1, -1), (-1, 1, -1), (-1, 1, 1)), red)
    sb.add_instance(q((1, -1, -1), (1, -1, 1), (1, 1, 1), (1, 1, -1)), white)
    if light:
        lamp = sb.add_material(Material(abi.RT_MAT_DIFFUSE, (0.78, 0.78, 0.78), emissive=(15.0, 15.0, 15.0)))
        sb.add_instance(q((-0.25, 0.995, -0.25), (0.25, 0.995, -0.25), (0.25, 0.995, 0.25), (-0.25, 0.995, 0.25)), lamp)
    sb.camera = CameraPose((0.0, 0.0, 3.4), (0.0, 0.0, -1.0), 2.0)
    return white


def room_scene():
    sb = SceneBuilder("room")
    _room(sb)
    return sb.build()


def planes_scene(gap):
    """a floor tessellated 6 x 6 and a second sheet `gap` above its middle: a ray that leaves the floor must still find the sheet"""
    sb = SceneBuilder(f"planes_{gap}")
    white = _room(sb)
    blue = sb.add_material(Material(abi.RT_MAT_DIFFUSE, (0.1, 0.2, 0.8)))
    sb.add_instance(sb.add_mesh(*mesh_quad((-0.9, -0.9, 0.9), (0.9, -0.9, 0.9), (0.9, -0.9, -0.9), (-0.9, -0.9, -0.9), nx=6, ny=6)), white)
    y = -0.9 + gap
    sb.add_instance(sb.add_mesh(*mesh_quad((-0.5, y, 0.5), (0.5, y, 0.5), (0.5, y, -0.5), (-0.5, y, -0.5), nx=3, ny=3)), blue)
    sb.camera = CameraPose((0.0, 0.6, 3.0), (0.0, -0.45, -1.0), 2.0)
    return sb.build()


def grazing_scene():
    """the camera looks along a tessellated floor at under 1 degree: mirror-like bounces leave it with |n . d| around the entries' thresholds"""
    sb = SceneBuilder("grazing")
    gloss = sb.add_material(Material(abi.RT_MAT_METALLIC, (0.9, 0.9, 0.9), roughness=0.02))
    white = sb.add_material(Material(abi.RT_MAT_DIFFUSE, (0.7, 0.7, 0.7)))
    sb.add_instance(sb.add_mesh(*mesh_quad((-4, 0, 4), (4, 0, 4), (4, 0, -4), (-4, 0, -4), nx=8, ny=8)), gloss)
    sb.add_instance(sb.add_mesh(*mesh_quad((-4, 0, -4), (4, 0, -4), (4, 3, -4), (-4, 3, -4), nx=2, ny=2)), white)
    sb.camera = CameraPose((0.0, 0.03, 3.9), (0.0, -0.008, -1.0), 1.2)  # atan(0.008) = 0.46 degrees
    return sb.build()


def slab_scene():
    sb = SceneBuilder("slab")
    _room(sb)
    glass = sb.add_material(Material(abi.RT_MAT_DIELECTRIC, ior=1.5))
    sb.add_instance(sb.add_mesh(*mesh_box()), glass, trs((0.0, -0.2, 0.0), s=(0.6, 0.5, 0.08)))
    return sb.build()


def column_scene():
    sb = SceneBuilder("column")
    white = _room(sb)
    sb.add_instance(sb.add_mesh(*mesh_cylinder(24, 6, radius=0.35, height=1.9)), white, trs((0.0, -0.98, 0.0)))
    return sb.build()


def bowl_scene(n=64, half=1.0, R=100.0, sign=+1, camera=None):
    """A shallow paraboloid y = sign (x^2 + z^2) / (2 R) over [-half, half]^2 (sign -1: a dome), n x n cells of two triangles: neighbours'
    normals differ by half / (n R) ~ 1.6e-4, inside the builder's 0.9 / 1024, so it names NEARLY flat subtrees — with a0 around 0.8, where the
    first term of the test refuses about half the rays of a wave and lets the others skip — and the tree is deep enough that most entries
    name a node trav_inner fetches from memory. From the default camera the renderers' own mirror bounces leave the bowl at |n . d| = 0.2 .. 0.6
    (the camera ray is about 2.1 long): they take the skip on leaf entries (a0 = 0.0016) and almost never on node entries (a0 = 0.79).
    `camera`: another pose — from straight above |n . d| is about 2 and the node entries are taken."""
    sb = SceneBuilder("bowl" if sign > 0 else "dome")
    metal = sb.add_material(Material(abi.RT_MAT_METALLIC, (0.9, 0.85, 0.7), roughness=0.1))
    white = sb.add_material(Material(abi.RT_MAT_DIFFUSE, (0.73, 0.73, 0.73)))
    lamp = sb.add_material(Material(abi.RT_MAT_DIFFUSE, (0.78, 0.78, 0.78), emissive=(15.0, 15.0, 15.0)))
    X, Z = np.meshgrid(np.linspace(-half, half, n + 1), np.linspace(-half, half, n + 1), indexing="xy")
    P = np.stack([X, sign * (X * X + Z * Z) / (2.0 * R), Z], -1)
    N = np.stack([-sign * X / R, np.ones_like(X), -sign * Z / R], -1)
    N /= np.linalg.norm(N, axis=-1, keepdims=True)
    idx = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            b, c, d = a + 1, a + n + 2, a + n + 1
            idx += [(a, c, b), (a, d, c)]  # (scenes.mesh_cylinder's layout: +y is the front)
    sb.add_instance(sb.add_mesh(P.reshape(-1, 3), N.reshape(-1, 3), np.stack([X, Z], -1).reshape(-1, 2), np.array(idx, np.uint32)), metal)
    sb.add_instance(sb.add_mesh(*mesh_quad((-1, 0, -1), (1, 0, -1), (1, 1, -1), (-1, 1, -1))), white)
    sb.add_instance(sb.add_mesh(*mesh_quad((-0.25, 1.5, -0.25), (0.25, 1.5, -0.25), (0.25, 1.5, 0.25), (-0.25, 1.5, 0.25))), lamp)
    sb.camera = camera or CameraPose((0.0, 0.4, 2.4), (0.0, -0.25, -1.0), 2.0)
    return sb.build()


def far_room_scene(offset):
    """The room turned off the axes and moved far from the origin THROUGH ITS TRANSFORMS (object-space positions stay small): a hit point
    origin + direction * t then lies up to half an ulp of |offset| off its wall, s = n . (o - p) is no longer 0 and the kSkipDist |s| term
    decides rays. (A move along one axis does not do it: the hit point on an axis-aligned wall rounds onto the plane exactly.)"""
    sd = scenes.rotate_scene(room_scene(), scenes.quat_axis_angle((1, 2, 3), 0.6))
    T = trs(tuple(float(v) for v in offset))
    sd.transforms = np.stack([scenes.mat4_mul(T, m) for m in sd.transforms]).astype(np.float32)  # (a translation: the normal matrices stay)
    sd.camera = CameraPose(tuple(float(p) + float(o) for p, o in zip(sd.camera.position, offset)), sd.camera.direction, sd.camera.focal_length)
    sd.name = "far_room_%g_%g_%g" % tuple(offset)
    return sd


def floor_scene(k):
    """the room with a k x k floor sheet: k = 28 puts the node count between what the two skip kernels stage (309) and kTopNodes (341),
    k = 32 just past kTopNodes"""
    sb = SceneBuilder(f"floor_{k}")
    white = _room(sb)
    sb.add_instance(sb.add_mesh(*mesh_quad((-0.9, -0.9, 0.9), (0.9, -0.9, 0.9), (0.9, -0.9, -0.9), (-0.9, -0.9, -0.9), nx=k, ny=k)), white)
    return sb.build()


NEW_CASES = {
    "bowl": bowl_scene,
    "dome": lambda: bowl_scene(sign=-1),
    "bowl_down": lambda: bowl_scene(camera=CameraPose((0.0, 1.2, 0.2), (0.0, -1.0, -0.15), 2.0)),
    "far_100": lambda: far_room_scene((100, 50, -200)),
    "far_300": lambda: far_room_scene((300, -200, 500)),
    "floor_28": lambda: floor_scene(28),
    "floor_32": lambda: floor_scene(32),
}
CASES = {  # every frame case of tests/test_gpu_origin_skip.py
    "room": room_scene,
    "planes_5e-5": lambda: planes_scene(5e-5),
    "planes_2e-4": lambda: planes_scene(2e-4),
    "planes_1e-3": lambda: planes_scene(1e-3),
    "grazing": grazing_scene,
    "slab": slab_scene,
    "column": column_scene,
    **NEW_CASES,
}

SCENES = {
    "atrium": lambda: scenes.atrium_scene(1),
    "cube": scenes.cube_scene,
    "cornell": scenes.cornell_scene,
    "voxel": lambda: scenes.voxel_scene(1),
    "atrium_tilted": lambda: scenes.atrium_tilted_scene(1, coarse=True),
    "atrium_rotated": lambda: scenes.atrium_tilted_scene(1, coarse=False),
    **NEW_CASES,
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


# ---- the per-ray test itself: which term decides, and the probe (rt_probe_origin_skip) against a float64 restatement ------------------------
def chain_rays(lib, sd, h, w=64, hh=48, gens=5, seed=11):
    """the bounce rays of a w x hh camera chain on the host walk, `gens` generations of _leave directions: (origins, directions, the triangle
    each ray starts on)"""
    tw = sd.world_triangles()
    rng = np.random.default_rng(seed)
    org, dirs = _camera_rays(lib, sd, w, hh)
    _, _, t, tri = _walk(lib, h, org, dirs, 0)
    O, D, S = [], [], []
    for _gen in range(gens):
        hit = tri != NONE
        if not hit.any():
            break
        d, start = dirs[hit], tri[hit]
        org = (org[hit] + (d * t[hit][:, None]).astype(np.float32)).astype(np.float32)
        dirs = _leave(_facing(tw, start, d), d, rng)
        O.append(org), D.append(dirs), S.append(start)
        _, _, t, tri = _walk(lib, h, org, dirs, 0)
    return np.concatenate(O), np.concatenate(D), np.concatenate(S)


def _half(bits):
    return np.ascontiguousarray(bits, np.uint32).astype(np.uint16).view(np.float16).astype(np.float64)


def skip_terms(entries, org, dirs):
    """rt_types.h: origin_skip_word restated in float64 on one entry (8 words) per ray: the three terms of the threshold, |n . d| and the tilt bound"""
    entries = np.ascontiguousarray(entries, np.uint32)
    n = entries[:, 1:4].copy().view(np.float32).astype(np.float64)
    p = entries[:, 4:7].copy().view(np.float32).astype(np.float64)
    w = org.astype(np.float64) - p
    d = dirs.astype(np.float64)
    with np.errstate(all="ignore"):
        t0 = _half(entries[:, 7] & 0xFFFF)
        t1 = K_SKIP_DIST * np.abs(np.sum(n * w, 1))
        t2 = _half(entries[:, 7] >> 16) * np.abs(w).sum(1)
        nd = np.abs(np.sum(n * d, 1))
        tilt = K_SKIP_TILT * np.abs(d).sum(1)
    return dict(ref=entries[:, 0], t0=t0, t1=t1, t2=t2, thr=t0 + t1 + t2, nd=nd, tilt=tilt)


def shares(m):
    """of the rays: skip taken, refused by a0, refused by the distance term (refused by a term: the tilt condition passes, the threshold
    does not, and the term is the largest of the three)"""
    named = m["ref"] != SKIP_NONE
    tilt_ok = named & (m["nd"] > m["tilt"])
    refused = tilt_ok & ~(m["nd"] > m["thr"])
    by_a0 = refused & (m["t0"] >= m["t1"]) & (m["t0"] >= m["t2"])
    by_dist = refused & (m["t1"] > m["t0"]) & (m["t1"] >= m["t2"])
    return float((tilt_ok & ~refused).mean()), float(by_a0.mean()), float(by_dist.mean())


def probe(lib, entries, org, dirs, device=-1):
    """rt_probe_origin_skip: (device words | None, host words)"""
    entries, org, dirs = np.ascontiguousarray(entries, np.uint32), np.ascontiguousarray(org, np.float32), np.ascontiguousarray(dirs, np.float32)
    n = org.shape[0]
    assert entries.shape == (n, 8) and org.shape == dirs.shape == (n, 3)
    host = np.full(n, 0xDEADBEEF, np.uint32)
    dev = np.full(n, 0xDEADBEEF, np.uint32) if device >= 0 else None
    abi.check(lib.rt_probe_origin_skip(device, n, abi.u32ptr(entries), abi.fptr(org), abi.fptr(dirs), abi.u32ptr(dev) if device >= 0 else None,
                                       abi.u32ptr(host)), lib)
    return dev, host


def build_case(devlib, name):
    """one of CASES built host only with the default tree (what Scene() renders from): its table, node count and chain rays"""
    sd = CASES[name]()
    c = sd.to_c()
    h = C.c_void_p()
    abi.check(devlib.rt_scene_create(C.byref(c), -1, abi.RT_BVH_DEFAULT, C.byref(h)), devlib)
    try:
        abi.check(devlib.rt_scene_check_bvh(h), devlib)
        words = _table(devlib, h)
        sc = [C.c_uint32(0) for _ in range(4)]
        bb, pad, bounds = C.c_int32(0), C.c_float(0), (C.c_float * 6)()
        abi.check(devlib.rt_dev_scene_tree(h, C.byref(sc[0]), C.byref(sc[1]), C.byref(sc[2]), C.byref(sc[3]), C.byref(bb), C.byref(pad), bounds,
                                           None, None, None, 0), devlib)
        org, dirs, start = chain_rays(devlib, sd, h)
    finally:
        devlib.rt_scene_destroy(h)
    return dict(sd=sd, words=words, n_nodes=sc[0].value, org=org, dirs=dirs, start=start)


def crafted_rays(case, seed=5, m=2000):
    """Rays ON the compares, for m named entries of a case: from a point of the entry's triangle, (first) a direction that leaves the
    surface scaled by thr / |n . d| x (1 + k 2^-23), k = -4 .. 4, so that |n . d| > thr straddles; (second) a direction at 1 / 256 elevation
    in the |d|_1 measure, its normal part scaled the same way, and long enough to pass the first compare. thr and the elevation are float64
    values of the model; what the fp32 test then says is for the host form to judge. -> (entries, origins, directions, first / second)"""
    rng = np.random.default_rng(seed)
    sd, words = case["sd"], case["words"]
    named = np.flatnonzero(words[:, 0] != SKIP_NONE)
    pick = rng.choice(named, size=m, replace=named.size < m)  # (a table of few entries: several points and directions per entry)
    tw = sd.world_triangles()[pick]
    b = rng.uniform(0, 1, size=(pick.size, 2))
    b = np.where((b.sum(1) > 1)[:, None], 1 - b, b)
    o = (tw[:, 0] + b[:, :1] * (tw[:, 1] - tw[:, 0]) + b[:, 1:] * (tw[:, 2] - tw[:, 0])).astype(np.float32)
    e = words[pick]
    n = e[:, 1:4].copy().view(np.float32).astype(np.float64)
    u = rng.uniform(-1, 1, size=n.shape)
    t = u - np.sum(u * n, 1, keepdims=True) * n
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    d0 = n * rng.uniform(0.3, 1.0, size=(pick.size, 1)) * rng.choice([-1.0, 1.0], size=(pick.size, 1)) + t * rng.uniform(0, 1, size=(pick.size, 1))
    m0 = skip_terms(e, o, d0)
    thr = np.maximum(m0["thr"], 1e-30)
    el = np.abs(t).sum(1) / 256
    for _ in range(3):
        el = np.abs(t + el[:, None] * n).sum(1) / 256
    long = 2.0 ** np.ceil(np.log2(np.maximum(1.0, 4 * thr / el)))
    E, O, D, kind = [], [], [], []
    for k in range(-4, 5):
        f = 1 + k * 2.0 ** -23
        E.extend([e, e]), O.extend([o, o]), kind.extend([np.zeros(pick.size, bool), np.ones(pick.size, bool)])
        D.append((d0 * (thr / m0["nd"] * f)[:, None]).astype(np.float32))
        D.append(((t + (el * f)[:, None] * n) * long[:, None]).astype(np.float32))
    return np.concatenate(E), np.concatenate(O), np.concatenate(D), np.concatenate(kind)


SYN_REF = 400 * 64  # a node past kTopNodes, as its parent stores it


def synthetic_cases():
    """Entries no scene would hold: (entries, origins, directions, the word exact arithmetic gives). Plane y = 0 through the origin unless said."""
    E, O, D, X = [], [], [], []
    f = lambda *v: np.array(v, np.float32)

    def add(want, d, a0=0, a2=0, o=(0, 0, 0), n=(0, 1, 0), p=(0, 0, 0)):
        e = np.zeros(8, np.uint32)
        e[0], e[7] = SYN_REF, a0 | (a2 << 16)
        e[1:4], e[4:7] = f(*n).view(np.uint32), f(*p).view(np.uint32)
        E.append(e), O.append(f(*o)), D.append(f(*d)), X.append(SYN_REF if want else SKIP_NONE)

    # thresholds that are half subnormals, 2^-24 x (1, 16, 1023): a device that flushed them to zero would skip on every one of these rays.
    # |n . d| = 5e-8 is below all three and above |d|_1 / 256; 5e-7 lies between the first and the second; 7e-5 is above all
    for a0, lo, mid, hi in ((0x0001, False, True, True), (0x0010, False, False, True), (0x03FF, False, False, True)):
        add(lo, (0, 5e-8, 0), a0), add(mid, (0, 5e-7, 0), a0), add(hi, (0, 7e-5, 0), a0)
        add(lo, (0, 5e-8, 0), 0, a0, o=(1, 0, 0)), add(mid, (0, 5e-7, 0), 0, a0, o=(0, 0, -1)), add(hi, (0, -7e-5, 0), 0, a0, o=(0.5, 0, 0.5))
    # the largest finite half (65504) and half infinity, as a0 and as a2 (times L = 1; times L = 0 infinity gives NaN: no skip)
    for kw in (dict(a0=0x7BFF), dict(a2=0x7BFF, o=(1, 0, 0))):
        add(True, (0, 1e5, 0), **kw), add(False, (0, 6e4, 0), **kw), add(True, (0, -65536, 0), **kw), add(False, (0, 65504, 0), **kw)
    for kw in (dict(a0=0x7C00), dict(a2=0x7C00, o=(1, 0, 0)), dict(a2=0x7C00)):
        add(False, (0, 1e5, 0), **kw), add(False, (0, 3e38, 0), **kw)
    # NaN and the infinities in every component of o, d, n and p in turn: never a skip
    base = dict(d=(0.3, 1.0, 0.2), a0=0x0400, a2=0x0400, o=(0.1, 0.0, 0.2), n=(0, 1, 0), p=(0.05, 0, 0.1))
    add(True, **base)
    for key in ("o", "d", "n", "p"):
        for i in range(3):
            for bad in (np.nan, np.inf, -np.inf):
                kw = dict(base)
                kw[key] = tuple(bad if j == i else v for j, v in enumerate(base[key]))
                add(False, **kw)
    # -0.0 components change nothing
    z = -0.0
    add(True, (z, 1, z), 0x0400, 0x0400, o=(z, z, z), n=(z, 1, z), p=(z, z, z))
    add(True, (z, -1, z), 0x0400, 0x0400, o=(z, z, z), n=(z, -1, z), p=(0, 0, 0))
    add(False, (z, z, z), 0x0400), add(False, (z, z, z)), add(False, (0, 0, 0))
    # subnormal directions: with thresholds of zero |n . d| = 1e-40 > 0 and > |d|_1 / 256 (a device that flushed fp32 subnormals would say no)
    add(True, (0, 1e-40, 0)), add(True, (1e-40, -1e-40, 1e-40)), add(False, (0, 1e-40, 0), 0x0001), add(False, (1e-37, 1e-40, 1e-37))
    # |d|_1 overflows: |n . d| = 3e38 is not above infinity / 256
    add(False, (2e38, 3e38, 2e38)), add(False, (-2e38, -3e38, 2e38)), add(True, (1e37, 3e38, 1e37))
    return np.stack(E), np.stack(O), np.stack(D), np.array(X, np.uint32)


@pytest.fixture(scope="module")
def cases(devlib):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = build_case(devlib, name)
        return cache[name]

    return get


def test_the_probe_is_exported_and_checks_its_arguments(rtlib, devlib):
    e, o, d, want = synthetic_cases()
    for lib in (rtlib, devlib):
        assert hasattr(lib, "rt_probe_origin_skip") and "rt_probe_origin_skip" in abi.PROTOTYPES
        w = np.zeros(1, np.uint32)
        assert lib.rt_probe_origin_skip(-1, 0, abi.u32ptr(e), abi.fptr(o), abi.fptr(d), None, abi.u32ptr(w)) == abi.RT_ERR_INVALID
        assert lib.rt_probe_origin_skip(-1, 1, None, abi.fptr(o), abi.fptr(d), None, abi.u32ptr(w)) == abi.RT_ERR_INVALID
        assert lib.rt_probe_origin_skip(-1, 1, abi.u32ptr(e), None, abi.fptr(d), None, abi.u32ptr(w)) == abi.RT_ERR_INVALID
        assert lib.rt_probe_origin_skip(-1, 1, abi.u32ptr(e), abi.fptr(o), None, None, abi.u32ptr(w)) == abi.RT_ERR_INVALID
        assert lib.rt_probe_origin_skip(-1, 1, abi.u32ptr(e), abi.fptr(o), abi.fptr(d), abi.u32ptr(w), None) == abi.RT_ERR_INVALID  # host only: no device word
        assert lib.rt_probe_origin_skip(-1, 1, abi.u32ptr(e), abi.fptr(o), abi.fptr(d), None, None) == abi.RT_OK
        np.testing.assert_array_equal(probe(lib, e, o, d)[1], want)


def test_every_term_is_at_work(cases):
    """Conditions on the INPUTS of the GPU tests, not measurements of the code: each of the three terms decides rays somewhere, and the table
    names nodes inside the staged top, in the 309 .. 340 band the two skip kernels stage no longer, past kTopNodes, and leaves."""
    got = {}
    for name in CASES:
        c = cases(name)
        got[name] = shares(skip_terms(c["words"][c["start"]], c["org"], c["dirs"]))
        print(f"{name}: {c['n_nodes']} nodes, {c['org'].shape[0]} chain rays, skip taken {got[name][0]:.3f}, refused by a0 {got[name][1]:.3f}, by the distance term {got[name][2]:.3f}")
    assert got["bowl"][0] >= 0.25 and got["bowl"][1] >= 0.10
    assert got["far_300"][2] >= 0.04 and got["far_300"][1] >= 0.15
    assert got["far_100"][2] >= 0.005
    ref = cases("bowl")["words"][:, 0]
    node = (ref != SKIP_NONE) & ((ref & 0x80000000) == 0)
    past, band, leaf = int((node & (ref >= K_TOP_NODES * 64)).sum()), int((node & (ref >= K_TOP_SKIP * 64) & (ref < K_TOP_NODES * 64)).sum()), int(((ref & 0x80000000) != 0).sum())
    a0 = _half(cases("bowl")["words"][ref != SKIP_NONE, 7] & 0xFFFF)
    print(f"bowl: {ref.size} triangles, {int((ref != SKIP_NONE).sum())} named: {past} name a node >= {K_TOP_NODES}, {band} one in {K_TOP_SKIP} .. {K_TOP_NODES - 1}, {leaf} a leaf; median a0 {np.median(a0):.2f}")
    assert past >= 1000 and band >= 1 and leaf >= 1000
    assert K_TOP_SKIP < cases("floor_28")["n_nodes"] <= K_TOP_NODES < cases("floor_32")["n_nodes"]


@pytest.mark.parametrize("name", list(CASES))
def test_the_host_form_of_the_probe_is_the_float64_model(devlib, cases, name):
    """origin_skip_word as the host compiler made it, on the chain rays of every case. A ray within 1e-5 (relative) of either compare is
    undecided and left out — at most 1 % of them; every other ray gets exactly the entry's word, or the no-match word, as the model says."""
    c = cases(name)
    e = c["words"][c["start"]]
    m = skip_terms(e, c["org"], c["dirs"])
    _, host = probe(devlib, e, c["org"], c["dirs"])
    close = lambda a, b: np.abs(a - b) <= 1e-5 * np.maximum(np.abs(a), np.abs(b))
    undecided = close(m["nd"], m["thr"]) | close(m["nd"], m["tilt"])
    want = np.where((m["nd"] > m["thr"]) & (m["nd"] > m["tilt"]), m["ref"], SKIP_NONE).astype(np.uint32)
    wrong = (host != want) & ~undecided
    print(f"{name}: {host.size} rays, {int(undecided.sum())} undecided ({100 * undecided.mean():.3f} %), {int((host != SKIP_NONE).sum())} skip, {int(wrong.sum())} differ from the model")
    assert undecided.mean() <= 0.01
    assert not wrong.any()


@pytest.mark.parametrize("name", list(CASES))
def test_crafted_rays_straddle_both_compares(devlib, cases, name):
    """the inputs of the GPU test's crafted set are worth their run: on the host form both compares come out both ways"""
    c = cases(name)
    e, o, d, second = crafted_rays(c)
    _, host = probe(devlib, e, o, d)
    taken = host != SKIP_NONE
    print(f"{name}: {host.size} crafted rays, skip on {taken[~second].mean():.3f} of those on the first compare, {taken[second].mean():.3f} of those on the tilt")
    assert 0.1 <= taken[~second].mean() <= 0.9 and 0.1 <= taken[second].mean() <= 0.9
