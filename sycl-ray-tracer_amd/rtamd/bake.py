"""A small vertex baker over gather queries (include/rt_mi355x.h: rt_gather_paths): the diffuse-lobe radiance at every triangle corner of a
scene. Pure Python over Scene.gather_paths; `albedo x result` is what the renderers show for a diffuse surface's first bounce there.
Beside it the helpers over the other queries: probe grids and clearance (closest points), reflection lookups, and the crossing count and
parity along rays (multi-hit queries: crossings, inside_mask), and the triangles within a radius and their contact points (k-nearest
closest-point queries: triangles_within, contact_points), and vertex ambient occlusion with its bent normal (occlusion gathers: bake_vertex_ao,
normalise_bent)."""
from __future__ import annotations

import numpy as np

from .renderer import Scene
from .scenes import SceneDesc

f32 = np.float32


def vertex_points(sd: SceneDesc):
    """The world-space corners of every triangle: (pos (T, 3, 3) float32, normal (T, 3, 3) float32), [triangle, corner, xyz].
    Positions with the scene builder's expression ((m0*x + m4*y) + m8*z) + m12 in fp32 (csrc/scene_build.cpp); normals are the vertex
    normals through the instance's normal matrix (column-major 3x3, the shading's expression), normalised, in fp32."""
    idx = np.asarray(sd.indices, np.int64).reshape(-1, 3)
    inst = np.asarray(sd.tri_instance, np.int64)
    m = np.asarray(sd.transforms, f32).reshape(-1, 16)[inst][:, None, :]    # (T, 1, 16)
    nm = np.asarray(sd.normal_mats, f32).reshape(-1, 9)[inst][:, None, :]   # (T, 1, 9)
    p = np.asarray(sd.positions, f32)[idx]                                  # (T, 3, 3)
    n = np.asarray(sd.normals, f32)[idx]
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    pos = np.stack([((m[..., r] * x + m[..., 4 + r] * y) + m[..., 8 + r] * z) + m[..., 12 + r] for r in range(3)], -1)
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    g = np.stack([(nm[..., r] * x + nm[..., 3 + r] * y) + nm[..., 6 + r] * z for r in range(3)], -1)
    inv = f32(1.0) / np.sqrt((g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2])
    nrm = g * inv[..., None]
    assert pos.dtype == f32 and nrm.dtype == f32
    return np.ascontiguousarray(pos), np.ascontiguousarray(nrm)


def corner_seeds(n_corners: int, repeats: int, seed: int) -> np.ndarray:
    """One xorshift32 state per (corner, repeat), (n_corners, repeats) uint32: a Weyl sequence from `seed`, never 0 (the state xorshift
    cannot leave)."""
    k = np.arange(n_corners * repeats, dtype=np.uint64) + np.uint64(1)
    s = ((np.uint64(seed & 0xFFFFFFFF) + k * np.uint64(0x9E3779B9)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    s[s == 0] = np.uint32(0x9E3779B9)
    return s.reshape(n_corners, repeats)


def bake_vertices(scene: Scene, sd: SceneDesc, samples: int, max_depth: int, seed: int, repeats: int = 1) -> np.ndarray:
    """The gathered radiance at every triangle corner, (T, 3, 3) float32 [triangle, corner, rgb]: one gather_paths call over 3T x repeats
    entries (corner-major, the repeats of a corner side by side, each with a state of its own from corner_seeds), the repeats averaged in
    fp32 in order. An entry is one lane's sequential work, so `repeats` is how a small mesh fills the device: samples x repeats paths per
    corner in all."""
    if repeats < 1:
        raise ValueError("repeats must be at least 1")
    pos, nrm = vertex_points(sd)
    c = pos.shape[0] * 3
    states = corner_seeds(c, repeats, seed)
    out = scene.gather_paths(np.repeat(pos.reshape(c, 3), repeats, axis=0), np.repeat(nrm.reshape(c, 3), repeats, axis=0), states.reshape(-1),
                             max_depth, samples=samples)
    rad = out["radiance"].reshape(c, repeats, 3)
    total = np.zeros((c, 3), f32)
    for k in range(repeats):
        total = total + rad[:, k]
    return (total / f32(repeats)).reshape(-1, 3, 3)


def normalise_bent(bent) -> np.ndarray:
    """The direction of a bent normal, (..., 3) float32: bent * (1 / sqrt((x*x + y*y) + z*z)) in fp32, and zero where bent is zero (an
    entry that is fully occluded has no unoccluded direction)."""
    b = np.asarray(bent, f32)
    if b.ndim < 1 or b.shape[-1] != 3:
        raise ValueError("bent must be (..., 3)")
    l2 = (b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1]) + b[..., 2] * b[..., 2]
    zero = (b == 0).all(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(zero[..., None], f32(0.0), b * (f32(1.0) / np.sqrt(l2))[..., None])
    assert out.dtype == f32
    return np.ascontiguousarray(out)


def bake_vertex_ao(scene: Scene, sd: SceneDesc, samples: int, max_dist, seed: int, repeats: int = 1):
    """Ambient occlusion at every triangle corner: (visibility (T, 3) float32, bent (T, 3, 3) float32 [triangle, corner, xyz], the
    normalised bent normal, zero where nothing is unoccluded). One gather_occlusion call over 3T x repeats entries (corner-major, the
    repeats of a corner side by side, each with a state of its own from corner_seeds), shaped as bake_vertices is; the repeats' visibility
    and bent sums are averaged in fp32 in order. max_dist: one distance in world units, or None (+inf)."""
    if repeats < 1:
        raise ValueError("repeats must be at least 1")
    pos, nrm = vertex_points(sd)
    c = pos.shape[0] * 3
    states = corner_seeds(c, repeats, seed)
    out = scene.gather_occlusion(np.repeat(pos.reshape(c, 3), repeats, axis=0), np.repeat(nrm.reshape(c, 3), repeats, axis=0), states.reshape(-1),
                                 samples, max_dist)
    vis, bent = out["visibility"].reshape(c, repeats), out["bent"].reshape(c, repeats, 3)
    tv, tb = np.zeros(c, f32), np.zeros((c, 3), f32)
    for k in range(repeats):
        tv, tb = tv + vis[:, k], tb + bent[:, k]
    return (tv / f32(repeats)).reshape(-1, 3), normalise_bent(tb / f32(repeats)).reshape(-1, 3, 3)


def triangle_grid_uvs(n_triangles: int, width: int, height: int, gutter: int = 1) -> np.ndarray:
    """A trivial lightmap unwrap for a width x height atlas (renderer.Lightmap), (n_triangles, 3, 2) float32: the atlas is cut into square
    cells of s x s texels, s the largest side at which every triangle gets a cell of its own (row-major, triangle t in cell t), and triangle t
    is the right triangle on its cell's low corner, inset by `gutter` texels on every side: corners (g, g), (s - g, g), (g, s - g) from the
    cell's origin, in texels, divided by the atlas size in fp32. Raises ValueError where s - 2 * gutter would be under 2 texels: such a
    triangle could miss every texel centre. It ignores the triangles' shapes: a way to bake and test scenes without lightmap UVs, not a
    chart packer."""
    n, w, h, g = int(n_triangles), int(width), int(height), int(gutter)
    if n < 0 or w < 1 or h < 1 or g < 0:
        raise ValueError("n_triangles and gutter must not be negative, width and height at least 1")
    if n == 0:
        return np.zeros((0, 3, 2), f32)
    s = min(w, h)
    while s >= 1 and (w // s) * (h // s) < n:
        s -= 1
    if s - 2 * g < 2:
        raise ValueError(f"{n} triangles in a {w} x {h} atlas get cells of {max(s, 0)} texels: under 2 inside a gutter of {g}")
    cols = w // s
    t = np.arange(n)
    ox, oy = (t % cols) * s, (t // cols) * s
    px = np.stack([ox + g, ox + s - g, ox + g], 1).astype(f32)
    py = np.stack([oy + g, oy + g, oy + s - g], 1).astype(f32)
    uv = np.stack([px / f32(w), py / f32(h)], 2)
    assert uv.dtype == f32
    return np.ascontiguousarray(uv)


def probe_grid(sd: SceneDesc, spacing: float, margin: float = 0.0):
    """A probe grid for renderer.ProbeVolume fitted to the scene's bounds: (origin (3,) float32, count (3,) of int). The probes start
    `margin` inside the low corner of the world triangles' bounds and step by `spacing` while they stay `margin` inside the high corner; an
    axis thinner than 2 * margin gets one probe at its middle. Raises ValueError where an axis would need more than 256 probes."""
    if not spacing > 0 or margin < 0:
        raise ValueError("spacing must be above 0, margin not negative")
    v = np.asarray(sd.world_triangles(), np.float64).reshape(-1, 3)
    if len(v) == 0:
        raise ValueError("the scene has no triangles to fit a grid to")
    lo, hi = v.min(0) + margin, v.max(0) - margin
    thin = hi < lo
    lo = np.where(thin, 0.5 * (lo + hi), lo)
    count = np.where(thin, 1, np.floor((hi - lo) / spacing + 1e-9).astype(np.int64) + 1)
    if (count > 256).any():
        raise ValueError(f"spacing {spacing} needs {int(count.max())} probes on an axis: 256 at most")
    return lo.astype(f32), tuple(int(c) for c in count)


def grid_points(origin, spacing, count) -> np.ndarray:
    """The points of a count[0] x count[1] x count[2] grid, (points, 3) float32: origin + (float)i * spacing per axis, one fp32 multiply
    and one add, in the probe volume's order p = (iz * count[1] + iy) * count[0] + ix (renderer.ProbeVolume.positions). `spacing` is one
    number or one per axis."""
    origin, spacing, count = np.asarray(origin, np.float64), np.asarray(spacing, np.float64), np.asarray(count)
    if spacing.ndim == 0:
        spacing = np.repeat(spacing, 3)
    if origin.shape != (3,) or spacing.shape != (3,):
        raise ValueError("origin must hold 3 numbers, spacing 1 or 3")
    if count.shape != (3,) or count.dtype.kind not in "ui" or (count < 0).any():
        raise ValueError("count must hold 3 integers, none negative")
    iz, iy, ix = np.meshgrid(*(np.arange(int(c)) for c in count[::-1]), indexing="ij")
    idx = np.stack([ix, iy, iz], -1).reshape(-1, 3).astype(f32)
    return np.ascontiguousarray(origin.astype(f32)[None, :] + idx * spacing.astype(f32)[None, :])


def distance_grid(scene: Scene, origin, spacing, count, max_dist=None):
    """The distance from every point of a grid to the scene's nearest triangle: (dist (cz, cy, cx) float32, tri (cz, cy, cx) uint32), one
    Scene.closest_points call over grid_points(origin, spacing, count). With a ProbeVolume's own origin, spacing and count it is the
    clearance of the volume's probes, in their order. max_dist: a radius beyond which a point is a miss (dist +inf, tri 0xFFFFFFFF)."""
    pts = grid_points(origin, spacing, count)
    shape = tuple(int(c) for c in np.asarray(count)[::-1])
    out = scene.closest_points(pts, max_dist)
    return out["dist"].reshape(shape), out["tri"].reshape(shape)


def triangles_within(scene: Scene, pos, radius):
    """The triangles within `radius` (one number or one per point) of every point, CSR (offsets (n + 1,) int64, tri uint32): point i's are
    tri[offsets[i]:offsets[i + 1]], in ascending (dist2, index) order — the set { j : dist2_j <= radius * radius } of Scene.closest_all,
    the radius squared in fp32."""
    if radius is None:
        raise ValueError("radius must be a number or one per point")
    out = scene.closest_all(pos, radius)
    return out[0], out[4]


def contact_points(wverts, pos, u, v, tri) -> np.ndarray:
    """The closest points that go with a k-nearest answer, re-formed from the vertices: the contract's point = p - r with
    r = (ap - u*e1) - v*e2 on the record (v0, v1 - v0, v2 - v0), every operation one fp32 operation (include/rt_mi355x.h:
    rt_point_query). wverts (T, 3, 3) float32 world vertices in global triangle order (vertex_points(sd)[0]); pos (n, 3); u, v, tri (n,)
    or (n, k) as Scene.closest_points_multi returns them. -> (n, 3) or (n, k, 3) float32, NaN where tri is 0xFFFFFFFF (a miss)."""
    wverts, pos = np.asarray(wverts), np.asarray(pos)
    u, v, tri = np.asarray(u), np.asarray(v), np.asarray(tri)
    if wverts.ndim != 3 or wverts.shape[1:] != (3, 3):
        raise ValueError("wverts must be (T, 3, 3)")
    if pos.ndim != 2 or pos.shape[1] != 3:
        raise ValueError("pos must be (n, 3)")
    if tri.ndim not in (1, 2) or tri.shape[0] != pos.shape[0] or u.shape != tri.shape or v.shape != tri.shape or tri.dtype.kind not in "iu":
        raise ValueError("u, v and tri must all be (n,) or (n, k), tri integers")
    wverts, pos = wverts.astype(f32, copy=False), pos.astype(f32, copy=False)
    u, v = u.astype(f32, copy=False)[..., None], v.astype(f32, copy=False)[..., None]
    hit = tri != 0xFFFFFFFF
    if hit.any() and int(tri[hit].max()) >= len(wverts):
        raise ValueError("tri holds an index past the last triangle")
    w = wverts[np.where(hit, tri, 0).astype(np.int64)] if len(wverts) else np.zeros(tri.shape + (3, 3), f32)
    p = pos if tri.ndim == 1 else pos[:, None, :]
    ap = p - w[..., 0, :]
    r = (ap - u * (w[..., 1, :] - w[..., 0, :])) - v * (w[..., 2, :] - w[..., 0, :])
    with np.errstate(invalid="ignore"):
        out = np.where(hit[..., None], p - r, f32(np.nan))
    assert out.dtype == f32
    return out


def crossings(scene: Scene, org, dirs, tmax=None) -> np.ndarray:
    """The number of surfaces along each ray, (n,) int64: the counting hits of Scene.trace_all (1e-4 < t <= tmax, every triangle once). A
    ray through an edge two triangles share counts both. On a mesh with ill-conditioned triangles (slivers) the count can be one short for
    a ray that hits one: trace_all's limit, stated there and in include/rt_mi355x.h."""
    offsets = scene.trace_all(org, dirs, tmax)[0]
    return np.diff(offsets)


def inside_mask(scene: Scene, points, direction) -> np.ndarray:
    """Odd crossing parity along one direction from every point, (n,) bool: crossings(points, direction) % 2 == 1. This means "inside" ONLY
    for a closed mesh, and only for rays that meet no edge and no vertex: an open mesh has no inside, and a ray through a shared edge or a
    vertex counts each triangle there (two or more for one surface crossing), one that grazes a silhouette edge may count one. Nothing here
    detects either case; a caller who must know compares two or three directions. A third case flips the parity as well: a ray that hits
    an ill-conditioned triangle (a sliver) can have that crossing missing (crossings' limit)."""
    points, direction = np.asarray(points), np.asarray(direction, f32)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError("points must be (n, 3)")
    if direction.shape != (3,):
        raise ValueError("direction must hold 3 numbers")
    dirs = np.ascontiguousarray(np.broadcast_to(direction, points.shape))
    return crossings(scene, points, dirs) % 2 == 1


def shade_vertices_from_volume(volume, sd: SceneDesc) -> np.ndarray:
    """bake_vertices' counterpart for a mesh that is NOT in the baked scene: the probe volume's irradiance over pi at every triangle corner
    of `sd` for its shading normal, (T, 3, 3) float32 [triangle, corner, rgb], one ProbeVolume.sample call over vertex_points(sd)."""
    pos, nrm = vertex_points(sd)
    return volume.sample(pos.reshape(-1, 3), nrm.reshape(-1, 3)).reshape(-1, 3, 3)


def lod_for_roughness(levels: int, roughness):
    """The level of detail of a renderer.ReflectionProbes chain for a surface roughness a in [0, 1], float32, one per roughness: the Phong
    exponent 2 / a^2 - 2 matched against the levels' lobes. Level l >= 1 is prefiltered with cos^(2^q_l), q_l = 2 * (levels - l) - 1, a power
    a quarter of the level's below, and level 0 continues that sequence (q_0 = 2 * levels - 1: its texels are the lobe); between two levels
    the lod is linear in log2 of the exponent, below the last level's power it is levels - 1, above level 0's it is 0. Host arithmetic in
    float64, outside the bit-exact contract."""
    if int(levels) < 1:
        raise ValueError("levels must be at least 1")
    a = np.clip(np.asarray(roughness, np.float64), 0.0, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.log2(np.maximum(2.0 / (a * a) - 2.0, 0.0))  # a = 0: +inf, a = 1: -inf
    return np.clip(int(levels) - 0.5 * (q + 1.0), 0.0, float(int(levels) - 1)).astype(f32)


def reflect_dirs(view, normal) -> np.ndarray:
    """view - 2 * dot(view, normal) * normal per row, (n, 3) float32: the direction ReflectionProbes.sample looks up for a view vector that
    points at the surface and a unit normal."""
    view, normal = np.asarray(view, f32), np.asarray(normal, f32)
    if view.ndim != 2 or view.shape[1] != 3 or normal.shape != view.shape:
        raise ValueError("view and normal must both be (n, 3)")
    d = (view * normal).sum(1, dtype=f32)
    return np.ascontiguousarray(view - (f32(2.0) * d)[:, None] * normal)
