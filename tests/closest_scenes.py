"""Scenes, points and radii for the closest-point tests on trees the kernel's own inner and leaf steps have to get right:
deep stacks, NaN candidates and slivers in deep leaves, pre-split triangles, duplicate triangles, scenes away from the origin, points in
the corner of the contract range, radii on an answer of zero. A plain module, imported by tests/test_closest_points.py (the host statement)
and tests/test_gpu_closest_points_trees.py (the device). Everything is seeded and built with tri_scene, so world vertices equal positions."""
import numpy as np

from rtamd import abi, scenes
from test_closest_points import NO_TRI, bounds_of, tri_scene

f32 = np.float32
FLT_MIN = np.finfo(f32).tiny
K_LDS_STACK = 12      # rt_device.h: kLdsStack, the entries of a lane's stack that live in LDS
K_TOP_NODES = 341     # rt_types.h: kTopNodes, the nodes a workgroup stages in LDS
OFFSETS = ((1000.0, -2000.0, 500.0), (1e5, 1e5, 1e5))
BUILDERS = {"sah": abi.RT_BVH_SAH, "lbvh": abi.RT_BVH_LBVH, "lbvh_gpu": abi.RT_BVH_LBVH_GPU}


def radius_mix(free_d2, seed):
    """per-entry squared radii around the unbounded answer: a fifth each exactly on it, the next float below it, twice it, a tenth of it,
    and +inf — with a few negative, -0.0 and 0 entries"""
    g = np.random.default_rng(seed)
    n = len(free_d2)
    kind = g.integers(0, 5, n)
    md2 = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [free_d2, np.nextafter(free_d2, f32(-np.inf)), f32(2) * free_d2, f32(0.1) * free_d2],
                    f32(np.inf)).astype(f32)
    md2[:3] = np.array([-1.0, -0.0, 0.0], f32)[:min(n, 3)]
    return md2


def pile_vertices(n=8192):
    """the vertex array of test_gpu_parity.py: test_deep_traversal_stacks_spill_and_equal_the_oracle, (n, 3, 3) float32"""
    z = -np.arange(n, dtype=f32) / f32(n)
    pos = np.zeros((n, 3, 3), f32)
    pos[:, 0] = (5.0, -5.0, 0.0)   # the hypotenuse: the same for both kinds
    pos[:, 1] = (-5.0, 7.0, 0.0)
    pos[:, 2] = (-5.0, -5.0, 0.0)  # kind B: covers 12 x + 10 y < 10, NOT the free corner (x, y in 1.5 .. 3)
    pos[[5, n - 6], 2] = (5.0, 7.0, 0.0)  # kind A: the other half of the same box
    pos[:, :, 2] = z[:, None]
    return pos


def pile_scene():
    """8,192 large parallel triangles with one bounding box: a point with no radius enters every child on its first descent, three pushes
    per level, past the 12 LDS entries of its stack"""
    return tri_scene("pile", pile_vertices())


def pile_corner_points(n, seed):
    """points in the free corner above and below the pile (x, y in 1.5 .. 3): nearest to the two triangles that cover the corner or to the
    hypotenuse of a great many others"""
    g = np.random.default_rng(seed)
    p = np.stack([g.uniform(1.5, 3.0, n), g.uniform(1.5, 3.0, n), g.uniform(0.5, 3.0, n)], -1)
    p[n // 2:, 2] = g.uniform(-3.0, -1.5, n - n // 2)
    return np.ascontiguousarray(p, f32)


def offset_scene(off):
    """the atrium at detail 1, its fp32 world triangles moved by `off`: the scene scale is the offset's, not the extent's"""
    tris = scenes.get_scene("atrium", detail=1).world_triangles().astype(f32) + np.asarray(off, f32)
    return tri_scene("atrium_off", tris)


def mixed_vertices(degenerate=True):
    """-> ((T, 3, 3) float32, (T,) bool: the degenerate triangles). default_rng(3), in this order: two scene-spanning triangles, 3,000 tiny
    ones (1e-6 .. 1e-2), 500 slivers (a, a + d, a + d / 2 + 1e-5 normal), 300 degenerate ones of three kinds by index % 3 — (a, a, b) with
    e1 = 0, whose edge region divides 0 by 0: the NaN source; (a, (a + b) / 2, b), collinear; (a, a, a), a point; b = a + 0.05 normal —
    all of it shuffled by one permutation."""
    g = np.random.default_rng(3)
    span = np.array([[[-1, -1, -1], [1, -1, 1], [-1, 1, 1]], [[1, 1, 1], [-1, 1, -1], [1, -1, -1]]], np.float64)
    c = g.uniform(-1.0, 1.0, (3000, 1, 3))
    tiny = c + g.normal(size=(3000, 3, 3)) * 10.0 ** g.uniform(-6.0, -2.0, (3000, 1, 1))
    a = g.uniform(-1.0, 1.0, (500, 3))
    d = g.normal(size=(500, 3))
    sliver = np.stack([a, a + d, a + 0.5 * d + 1e-5 * g.normal(size=(500, 3))], 1)
    parts = [span, tiny, sliver]
    if degenerate:
        a = g.uniform(-1.0, 1.0, (300, 3))
        b = a + 0.05 * g.normal(size=(300, 3))
        kind = (np.arange(300) % 3)[:, None, None]
        parts.append(np.where(kind == 0, np.stack([a, a, b], 1), np.where(kind == 1, np.stack([a, 0.5 * (a + b), b], 1), np.stack([a, a, a], 1))))
    tris = np.concatenate(parts).astype(f32)
    mask = np.zeros(len(tris), bool)
    if degenerate:
        mask[-300:] = True
    perm = g.permutation(len(tris))
    return np.ascontiguousarray(tris[perm]), mask[perm]


def mixed_scene(degenerate=True):
    """-> (scene, mask of the degenerate triangles' indices)"""
    tris, mask = mixed_vertices(degenerate)
    return tri_scene("mixed", tris), mask


def nan_source(tris, mask):
    """the indices of the degenerate triangles of kind 0, (a, a, b): v1 == v0 and v2 != v0"""
    return np.flatnonzero(mask & (tris[:, 0] == tris[:, 1]).all(1) & (tris[:, 0] != tris[:, 2]).any(1))


DUPLICATE_COPIES = 7


def duplicate_order():
    """scene index -> index into the cube's twelve triangles tiled DUPLICATE_COPIES times"""
    return np.random.default_rng(3).permutation(12 * DUPLICATE_COPIES)


def duplicate_scene():
    """the cube's 12 world triangles seven times, shuffled: every candidate ties with six others bit for bit, and the lowest index wins"""
    cube = scenes.get_scene("cube").world_triangles().astype(f32).reshape(12, 3, 3)
    return tri_scene("duplicates", np.tile(cube, (DUPLICATE_COPIES, 1, 1))[duplicate_order()])


def lowest_copy(tri):
    """For winners `tri` on duplicate_scene(): the lowest scene index among the copies of each winner's triangle, from the permutation
    alone. Scene index i holds the cube's triangle duplicate_order()[i] % 12."""
    which = duplicate_order() % 12
    first = np.array([np.flatnonzero(which == k)[0] for k in range(12)], np.uint32)
    assert (tri != NO_TRI).all()
    return first[which[tri]]


def contract_limits(sd):
    """(lo, hi, limit) in fp32 as rt_frame.hip: contract_range forms them from the fp32 world bounds (tri_scene: world vertices = positions)"""
    v = np.asarray(sd.world_triangles(), f32).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    scale = max(max(f32(hi[a] - lo[a]), max(abs(lo[a]), abs(hi[a]))) for a in range(3))
    return lo, hi, f32(100.0) * f32(scale)


def corner_points(sd, n, seed):
    """Points in the corner of the contract range: every axis outside on a random side, 99.9 scene scales x uniform(0.99, 1) beyond the
    bound (the limit is 100). Each is inside the range as rt_types.h: in_contract_range evaluates it in fp32."""
    g = np.random.default_rng(seed)
    lo, hi, scale = bounds_of(sd)
    out = 99.9 * scale * g.uniform(0.99, 1.0, (n, 3))
    below = g.integers(0, 2, (n, 3)) == 1
    pos = np.ascontiguousarray(np.where(below, lo - out, hi + out), f32)
    flo, fhi, limit = contract_limits(sd)
    outside = np.maximum(np.maximum(flo - pos, pos - fhi), f32(0.0))
    assert outside.dtype == f32 and (outside <= limit).all() and (outside > f32(98.0) * (limit / f32(100.0))).all()
    return pos


def vertex_radii(wv, n):
    """-> (pos, max_dist2): the first n world vertices as points, max_dist2 cycling through -0.0, +0.0, FLT_MIN, +inf (each admits the
    answer dist2 == 0) and -1 (a miss)"""
    pos = np.ascontiguousarray(np.asarray(wv, f32).reshape(-1, 3)[:n])
    assert len(pos) == n
    md2 = np.tile(np.array([-0.0, 0.0, FLT_MIN, np.inf, -1.0], f32), (n + 4) // 5)[:n]
    return pos, np.ascontiguousarray(md2)


def check_vertex_radii(out, pos, md2, what="", third_vertices=True):
    """What the contract says of vertex_radii's entries: -1 misses; every other radius hits with dist2 == 0 and the vertex as point.
    That holds for a triangle's v0 and v1 on every scene by the contract's own arithmetic: at v0, ap = 0 and the first region gives
    r = ap; at v1, ap is the record's e1 bit for bit (both are fl(v1 - v0)), so bp = 0, d3 = d4 = 0, the second region holds and
    r = (e1 - 1 * e1) - 0 * e2 = 0. At v2 it is the contract's stated limit: cp = 0 and d5 = d6 = 0, and the regions in front of the
    fourth decide on products that cancel. On a sliver the edge region of e1 wins (u ~ 0.5, dist2 ~ 1e-11 on the mixed scene), and on a
    triangle with e1 = 0 that region divides 0 by 0 and the candidate is NaN. third_vertices = False leaves the v2 entries (index % 3 ==
    2: the radii's cycle of five meets every vertex) to the comparison with the model: 453 of the mixed scene's 3,802 are not at 0."""
    miss = md2 == f32(-1.0)
    assert miss.sum() == len(pos) // 5 and np.signbit(md2[0::5]).all() and not np.signbit(md2[1::5]).any(), what
    assert (out["tri"][miss] == NO_TRI).all() and np.isinf(out["dist2"][miss]).all() and np.isnan(out["point"][miss]).all(), what
    zero = ~miss if third_vertices else ~miss & (np.arange(len(pos)) % 3 != 2)
    for r in (-0.0, 0.0, FLT_MIN, np.inf):
        assert (zero & (md2 == f32(r)) & (np.signbit(md2) == np.signbit(f32(r)))).sum() >= len(pos) // 10, (what, r)
    assert (out["tri"][zero] != NO_TRI).all() and (out["dist2"][zero] == 0).all(), what
    np.testing.assert_array_equal(out["point"][zero], pos[zero], err_msg=what)
