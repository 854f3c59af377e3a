"""The inner step's hit bookkeeping on lane masks (csrc/rt_device.h: trav_inner<true>) on the GPU. The one-launch kernels keep
"child k was hit" as four SGPR masks: `descend` and the three pushes are and / or of the masks; in k_wf_finish a missed child has no key
and the comparators swap on  hB & (~hA | lanes(KB < KA)),  in k_megakernel it keeps its +inf key for the swaps. None of that may change a
hit, a frame or a ray count, so everything here is held to the CPU oracle's brute force, bit for bit, by both renderers.

The scene is four open tubes of axis-aligned quads at exactly representable coordinates, pushed into each other along x so that their
boxes overlap: the host builder makes a root whose four children are all inner nodes (checked on the host tree; skipped with the reason if a
builder ever does otherwise), and there are places inside none, one, two, three and all four child boxes. The crafted rays start in each of
those, in every sign octant and along the axes, from outside with every box behind them, and from exactly on a decoded box plane looking in
and out, with tmax +inf, between the first and the second hit, and kTNear. They go through the closest-hit ray query — whose kernel keeps the
+inf keys (trav_inner<false>): the same tree, boxes and rays pin the step both texts must equal. The mask text itself runs in the two
one-launch renderers: the same scene from a camera on vertex coordinates inside it, a tile below a wave, the tilted atrium at depth 10, and
a stack of 1024 parallel sheets seen along its axis, where every box on a lane's way is pierced and its stack runs past the 12 LDS entries:
the general push / pop path, which branches on the same masks."""
import numpy as np
import pytest

from rtamd import abi
from rtamd.renderer import Camera, MegakernelRenderer, Scene, WavefrontRenderer
from rtamd.scenes import CameraPose, Material, SceneBuilder, mesh_quad
from test_gpu_ray_query import NO_TRI, assert_closest, expected, trace_dev

pytestmark = pytest.mark.gpu
f32 = np.float32
K_T_NEAR = f32(1e-4)
K_LDS_STACK = 12  # kLdsStack
KINDS = ((WavefrontRenderer, abi.RT_RENDERER_WAVEFRONT), (MegakernelRenderer, abi.RT_RENDERER_MEGAKERNEL))


def tubes_scene():
    """tube k: x in [2k, 2k + 8], y and z in [-1/2 + k/8, 1/2 + k/8], four walls and a partition across its middle: 20 quads"""
    sb = SceneBuilder("tubes")
    white = sb.add_material(Material(abi.RT_MAT_DIFFUSE, (0.73, 0.73, 0.73)))
    red = sb.add_material(Material(abi.RT_MAT_DIFFUSE, (0.65, 0.05, 0.05)))
    metal = sb.add_material(Material(abi.RT_MAT_METALLIC, (0.9, 0.85, 0.7), roughness=0.1))
    lamp = sb.add_material(Material(abi.RT_MAT_DIFFUSE, (0.78, 0.78, 0.78), emissive=(4.0, 4.0, 4.0)))
    q = lambda *a: sb.add_mesh(*mesh_quad(*a))
    for k in range(4):
        x0, x1, lo, hi = 2.0 * k, 2.0 * k + 8.0, -0.5 + k / 8.0, 0.5 + k / 8.0
        xm = 0.5 * (x0 + x1)
        sb.add_instance(q((x0, lo, hi), (x1, lo, hi), (x1, lo, lo), (x0, lo, lo)), white)
        sb.add_instance(q((x0, hi, lo), (x1, hi, lo), (x1, hi, hi), (x0, hi, hi)), lamp if k % 2 else white)
        sb.add_instance(q((x0, lo, lo), (x1, lo, lo), (x1, hi, lo), (x0, hi, lo)), red)
        sb.add_instance(q((x1, lo, hi), (x0, lo, hi), (x0, hi, hi), (x1, hi, hi)), metal)
        sb.add_instance(q((xm, lo, hi), (xm, lo, lo), (xm, hi, lo), (xm, hi, hi)), (white, red, metal)[k % 3])
    sb.camera = CameraPose((6.0, 0.125, -0.375), (1.0, 0.1, 0.2), 1.0)  # x: where tube 3 starts; y, z: wall coordinates of tube 1
    return sb.build()


def sheets_scene(n=1024):
    """n parallel sheets 1/64 apart along z, seen from in front along -z: every child box of every node on a ray's way is pierced"""
    sb = SceneBuilder("sheets")
    white = sb.add_material(Material(abi.RT_MAT_DIFFUSE, (0.73, 0.73, 0.73)))
    lamp = sb.add_material(Material(abi.RT_MAT_DIFFUSE, (0.78, 0.78, 0.78), emissive=(4.0, 4.0, 4.0)))
    for i in range(n):
        z = -i / 64.0
        sb.add_instance(sb.add_mesh(*mesh_quad((-1, -1, z), (1, -1, z), (1, 1, z), (-1, 1, z))), lamp if i % 7 == 3 else white)
    sb.camera = CameraPose((0.0, 0.0, 2.0), (0.0, 0.0, -1.0), 2.0)
    return sb.build()


def child_boxes(node):
    """the four boxes of a host node (16 uint32 words) as trav_inner decodes them: origin + q * scale, in fp32"""
    f = node.view(f32)
    org, sc = f[0:3], np.abs(np.array([f[3], f[10], f[11]], f32))
    lo, hi = np.zeros((4, 3), f32), np.zeros((4, 3), f32)
    for k in range(4):
        for a in range(3):
            lo[k, a] = org[a] + f32((node[4 + 2 * a] >> (8 * k)) & 0xFF) * sc[a]
            hi[k, a] = org[a] + f32((node[5 + 2 * a] >> (8 * k)) & 0xFF) * sc[a]
    return lo, hi


def host_tree(devlib, sd):
    s = Scene(sd, device=-1, lib=devlib)
    try:
        s.check_bvh()
        return s.tree()
    finally:
        s.close()


@pytest.fixture(scope="module")
def tubes(rtlib, devlib, oracle):
    assert rtlib.rt_device_count() > 0, "GPU tests need a device; the product has no CPU fallback"
    sd = tubes_scene()
    nodes = host_tree(devlib, sd)["nodes"]
    kids = nodes[0, 12:16].view(np.int32)
    if not (kids >= 0).all():
        pytest.skip(f"the builder's root has child words {kids.tolist()}: not four inner nodes, the crafted rays would not sort four hit boxes")
    scene = Scene(sd, device=0)
    yield sd, child_boxes(nodes[0]), scene, oracle.OracleScene(sd)
    scene.close()


def crafted_rays(sd, boxes):
    lo, hi = boxes
    rng = np.random.default_rng(3)
    xs = np.arange(-2.0, 16.5, 0.5)
    yz = np.arange(-0.75, 1.125, 0.125)
    grid = np.array(np.meshgrid(xs, yz, yz, indexing="ij"), f32).reshape(3, -1).T
    inside = ((grid[:, None, :] >= lo[None]) & (grid[:, None, :] <= hi[None])).all(-1).sum(1)
    octants = np.array([(sx, sy * 0.5, sz * 0.25) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], f32)
    axes = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], f32)
    dirs14 = np.concatenate([octants, axes])
    org, dirs, counts = [], [], {}
    for c in range(5):
        pts = grid[inside == c]
        counts[c] = len(pts)
        pts = pts[rng.permutation(len(pts))[:60]]
        org.append(np.repeat(pts, len(dirs14), axis=0)), dirs.append(np.tile(dirs14, (len(pts), 1)))
    # every box behind the ray: from beyond each corner of the scene, pointing further away
    tw = sd.world_triangles().reshape(-1, 3)
    slo, shi = tw.min(0), tw.max(0)
    for corner in octants:
        s = np.sign(corner)
        o = np.where(s > 0, shi + 1.0, slo - 1.0).astype(f32)
        away = np.array([corner, s, (s[0], 0, 0)], f32)
        org.append(np.tile(o, (3, 1))), dirs.append(away)
    n_away = 24
    # exactly on a decoded plane of a child box, the other two coordinates at the box's middle: looking in and out, straight and tilted
    for k in range(4):
        mid = ((lo[k] + hi[k]) * f32(0.5)).astype(f32)
        for a in range(3):
            for plane in (lo[k, a], hi[k, a]):
                o = mid.copy()
                o[a] = plane
                for sgn in (1.0, -1.0):
                    straight = np.zeros(3, f32)
                    straight[a] = sgn
                    tilted = np.array([0.25, 0.125, -0.125], f32)
                    tilted[a] = sgn
                    org.append(np.stack([o, o])), dirs.append(np.stack([straight, tilted]))
    n_plane = 4 * 3 * 2 * 2 * 2
    return np.concatenate(org).astype(f32), np.concatenate(dirs).astype(f32), counts, n_away, n_plane


def all_hits_f64(sd, org, dirs):
    """every t of every ray on every triangle, Moller-Trumbore in float64 (only to place a tmax between two hits; no judge of anything)"""
    tw = sd.world_triangles().astype(np.float64)
    v0, e1, e2 = tw[:, 0], tw[:, 1] - tw[:, 0], tw[:, 2] - tw[:, 0]
    o, d = org.astype(np.float64)[:, None, :], dirs.astype(np.float64)[:, None, :]
    p = np.cross(d, e2[None])
    det = (e1[None] * p).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        tv = o - v0[None]
        u = (tv * p).sum(-1) * inv
        qv = np.cross(tv, e1[None])
        v = (d * qv).sum(-1) * inv
        t = (e2[None] * qv).sum(-1) * inv
        ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 1e-3)
    return np.sort(np.where(ok, t, np.inf), axis=1)


def test_crafted_rays_through_the_closest_hit_query(tubes):
    sd, boxes, scene, osc = tubes
    org, dirs, counts, n_away, n_plane = crafted_rays(sd, boxes)
    assert all(counts[c] > 0 for c in range(5)), f"origins inside 0 .. 4 child boxes of the root: {counts}"
    assert len(org) > 4000
    e = osc.intersect(org, dirs, use_bvh=False)
    hit = e[3] != NO_TRI
    assert 0.3 < hit.mean() < 0.95
    away = slice(len(org) - n_plane - n_away, len(org) - n_plane)
    assert not hit[away].any()  # every box behind them
    assert_closest(scene.intersect(org, dirs), e, "rt_intersect_batch")
    assert_closest(scene.trace(org, dirs), e, "tmax +inf")
    assert_closest(trace_dev(scene, org, dirs), e, "tmax +inf, device entry")
    ts = all_hits_f64(sd, org, dirs)
    first = np.where(np.isfinite(ts[:, 0]), ts[:, 0], -1.0)
    two = np.isfinite(ts[:, 1]) & (ts[:, 1] > ts[:, 0] * 1.001) & hit & (np.abs(first - e[0]) <= 1e-4 * e[0])  # (the first is the oracle's)
    assert two.sum() > 500
    between = np.where(two, 0.5 * (ts[:, 0] + ts[:, 1]), np.where(hit, 1.5 * e[0], np.inf)).astype(f32)
    short = np.where(hit, 0.5 * e[0], 1.0).astype(f32)
    for what, tmax in (("between two hits", between), ("in front of the first hit", short), ("kTNear", np.full(len(org), K_T_NEAR))):
        ex = expected(e, tmax)
        assert_closest(scene.trace(org, dirs, tmax), ex[:4], what)
        np.testing.assert_array_equal(scene.trace(org, dirs, tmax, any_hit=True), ex[4], err_msg=what)
    assert expected(e, between)[4].sum() == hit.sum() and expected(e, short)[4].sum() == 0
    assert expected(e, np.full(len(org), K_T_NEAR))[4].sum() == 0


def _hold(scene, sd, osc, oracle, w, h, spp, depth, use_bvh=False):
    cam = Camera.for_scene(sd, (w, h))
    ocam = oracle.camera(w, h, sd.camera.position, sd.camera.direction, sd.camera.focal_length)
    for cls, kind in KINDS:
        f, b, rays = osc.render(ocam, kind, depth, spp, use_bvh=use_bvh)
        assert rays > w * h * spp  # paths do bounce
        r = cls(scene, (w, h), depth, spp)
        try:
            fr = r.render_frame(cam)
        finally:
            r.close()
        what = f"{sd.name} {w} x {h} {cls.__name__}"
        assert fr.rays == rays, f"{what}: {fr.rays} rays, the oracle {rays}"
        np.testing.assert_array_equal(fr.rgba_f32, f, err_msg=what)
        np.testing.assert_array_equal(fr.rgba_u8, b, err_msg=what)


@pytest.mark.parametrize("w,h,spp,depth", [(16, 16, 4, 5), (5, 3, 4, 5)])
def test_the_one_launch_renderers_from_inside_the_tubes(tubes, oracle, w, h, spp, depth):
    sd, _, scene, osc = tubes
    _hold(scene, sd, osc, oracle, w, h, spp, depth)


def test_the_one_launch_renderers_on_the_tilted_atrium(rtlib, oracle, scene_cache):
    sd = scene_cache("atrium_tilted", detail=1)
    scene = Scene(sd, device=0)
    try:
        _hold(scene, sd, oracle.OracleScene(sd), oracle, 64, 8, 3, 10, use_bvh=True)
    finally:
        scene.close()


def first_descent_stack(nodes, z0):
    """entries on the stack of a ray (0, 0, z0) -> -z when it reaches its first leaf: nearest hit child first, the other hit children pushed"""
    cur, depth = 0, 0
    while True:
        lo, hi = child_boxes(nodes[cur])
        kids = nodes[cur, 12:16].view(np.int32)
        hits = sorted((max(z0 - float(hi[k, 2]), 0.0), k) for k in range(4)
                      if kids[k] != -2 ** 31 and lo[k, 0] <= 0 <= hi[k, 0] and lo[k, 1] <= 0 <= hi[k, 1] and lo[k, 2] <= z0)
        if not hits:
            return depth
        depth += len(hits) - 1
        first = int(kids[hits[0][1]])
        if first < 0:
            return depth
        cur = first


def test_a_stack_past_its_lds_entries(rtlib, devlib, oracle):
    """the general push / pop path (stk_push / trav_pop under in_mask of the same masks)"""
    sd = sheets_scene()
    deep = first_descent_stack(host_tree(devlib, sd)["nodes"], float(sd.camera.position[2]))
    if deep <= K_LDS_STACK:
        pytest.skip(f"the builder's tree puts {deep} entries on the stack of a ray along the sheets' axis: not past the {K_LDS_STACK} in LDS")
    scene = Scene(sd, device=0)
    try:
        _hold(scene, sd, oracle.OracleScene(sd), oracle, 16, 16, 4, 5)
    finally:
        scene.close()
