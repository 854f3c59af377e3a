"""Lightmap baking (include/rt_mi355x.h: rt_lightmap_*) without a GPU: the numpy model of the contract's steps 1, 2, 3, 5 and 6 that
tests/test_gpu_lightmap.py compares the device with (owner_model, texel_model, entry_states, resolve_model, dilate_model), what the model
itself must show (no holes between triangles that share an edge, the tie on a diagonal through texel centres, the rings of a dilation, the
states, the trivial unwrap), and the library in front of the device: the exported symbols, the refusals, the wrappers' shape checks."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rtamd import abi, bake, scenes
from rtamd.renderer import Lightmap, Scene

REPO = Path(__file__).resolve().parent.parent
f32 = np.float32
NONE = 0xFFFFFFFF
SYMBOLS = ["rt_lightmap_create", "rt_lightmap_destroy", "rt_lightmap_texels", "rt_lightmap_texels_device", "rt_lightmap_bake",
           "rt_lightmap_bake_device"]
# the atlases the GPU tests lay the Cornell box's 116 triangles on (test_unwrap_gives_every_cornell_triangle_a_texel): cells of 5 and of 4
# texels with a gutter of 1, and for the chain over the CPU oracle 32 x 32 with cells of 2 and no gutter (width, height, gutter)
CORNELL_ATLASES = [(64, 64), (65, 33)]
CORNELL_ORACLE_ATLAS = (32, 32, 0)


# ---- the model both files share ---------------------------------------------------------------------------------------------------------
def _E(ax, ay, bx, by, qx, qy):
    """E(A, B, q) = (B.x - A.x) * (q.y - A.y) - (B.y - A.y) * (q.x - A.x) on float32 arrays: five fp32 operations"""
    return (bx - ax) * (qy - ay) - (by - ay) * (qx - ax)


def _edge(ix, iy, jx, jy, qx, qy):
    """the directed edge i -> j at q, evaluated from the corner that comes first (x, then y)"""
    first = (ix < jx) | ((ix == jx) & (iy <= jy))
    return np.where(first, _E(ix, iy, jx, jy, qx, qy), -_E(jx, jy, ix, iy, qx, qy))


def texel_space(lm_uv, W, H):
    """-> (P (T, 3, 2) float32, the corners in texel space, area (T,), ok (T,): six finite coordinates and area != 0)"""
    uv = np.asarray(lm_uv, f32).reshape(-1, 3, 2)
    with np.errstate(all="ignore"):
        P = uv * np.array([W, H], f32)
        area = _edge(P[:, 0, 0], P[:, 0, 1], P[:, 1, 0], P[:, 1, 1], P[:, 2, 0], P[:, 2, 1])
        ok = np.isfinite(P).all(axis=(1, 2)) & (area != 0)
    assert P.dtype == f32 and area.dtype == f32
    return P, area, ok


def edge_values(P, area, cx, cy):
    """e0, e1, e2 and the cover flag for corners P (..., 3, 2), areas (...) and centres cx, cy broadcast against them"""
    c = [(P[..., k, 0], P[..., k, 1]) for k in range(3)]
    with np.errstate(all="ignore"):
        e0 = _edge(*c[1], *c[2], cx, cy)
        e1 = _edge(*c[2], *c[0], cx, cy)
        e2 = _edge(*c[0], *c[1], cx, cy)
        pos = (e0 >= 0) & (e1 >= 0) & (e2 >= 0)
        neg = (e0 <= 0) & (e1 <= 0) & (e2 <= 0)
        cover = np.where(area > 0, pos, np.where(area < 0, neg, False))
    return e0, e1, e2, cover


_K = 8  # the batched boxes' side


def owner_model(lm_uv, W, H, full=False):
    """Step 1: every texel's owner, (W * H,) uint32, NONE where no triangle covers its centre. full: every triangle is tested at every
    texel, the contract as written; else at the texels of its box grown by a texel on every side (a superset of what can be covered, like
    the kernel's), the small boxes in one batch."""
    P, area, ok = texel_space(lm_uv, W, H)
    owner = np.full(W * H, NONE, np.uint32)
    tris = np.flatnonzero(ok)
    if len(tris) == 0:
        return owner
    Pk = P[tris].astype(np.float64)
    if full:
        x0, x1 = np.zeros(len(tris), np.int64), np.full(len(tris), W - 1, np.int64)
        y0, y1 = np.zeros(len(tris), np.int64), np.full(len(tris), H - 1, np.int64)
    else:
        def span(v, n):
            lo = np.clip(np.floor(np.clip(v.min(1), -4.0, n + 4.0) - 0.5) - 1, 0, n).astype(np.int64)
            hi = np.clip(np.floor(np.clip(v.max(1), -4.0, n + 4.0) - 0.5) + 1, -1, n - 1).astype(np.int64)
            return lo, hi
        x0, x1 = span(Pk[:, :, 0], W)
        y0, y1 = span(Pk[:, :, 1], H)
    bw, bh = x1 - x0 + 1, y1 - y0 + 1
    live = (bw > 0) & (bh > 0)
    small = live & (bw <= _K) & (bh <= _K) & (not full)
    s = np.flatnonzero(small)
    if len(s):
        k = np.arange(max(bw[s].max(), bh[s].max()))
        xs, ys = x0[s, None] + k, y0[s, None] + k                                   # (S, K)
        inside = (xs <= x1[s, None])[:, None, :] & (ys <= y1[s, None])[:, :, None]  # (S, K rows, K columns)
        cx = (xs.astype(f32) + f32(0.5))[:, None, :]
        cy = (ys.astype(f32) + f32(0.5))[:, :, None]
        t = tris[s]
        cover = edge_values(P[t][:, None, None], area[t][:, None, None], cx, cy)[3] & inside
        a, r, c = np.nonzero(cover)
        np.minimum.at(owner, ys[a, r] * W + xs[a, c], t[a].astype(np.uint32))
    for j in np.flatnonzero(live & ~small):
        t = tris[j]
        xs, ys = np.arange(x0[j], x1[j] + 1), np.arange(y0[j], y1[j] + 1)
        cover = edge_values(P[t], area[t], (xs.astype(f32) + f32(0.5))[None, :], (ys.astype(f32) + f32(0.5))[:, None])[3]
        r, c = np.nonzero(cover)
        idx = ys[r] * W + xs[c]
        owner[idx] = np.minimum(owner[idx], np.uint32(t))
    return owner


def shading_inputs(sd):
    """What step 2 reads of a scene description: (wv (T, 9) float32, the world-space vertices in the scene builder's expression
    (bake.vertex_points), n (T, 3, 3) float32, the corners' object-space normals, nm (T, 9) float32, the instance's normal matrix)"""
    with np.errstate(all="ignore"):  # its corner normals, not used here, divide by zero on a mesh with zero normals
        wv = bake.vertex_points(sd)[0].reshape(-1, 9)
    idx = np.asarray(sd.indices, np.int64).reshape(-1, 3)
    n = np.asarray(sd.normals, f32)[idx]
    nm = np.asarray(sd.normal_mats, f32).reshape(-1, 9)[np.asarray(sd.tri_instance, np.int64)]
    return wv, n, nm


def _normalize(x, y, z):
    with np.errstate(all="ignore"):
        inv = f32(1.0) / np.sqrt((x * x + y * y) + z * z)
        return x * inv, y * inv, z * inv


def texel_model(sd, lm_uv, W, H, owner):
    """Step 2: (pos (W * H, 3) float32, normal (W * H, 3) float32) of every texel for its owner; NaN (0x7FC00000) and 0 where empty"""
    P, area, _ = texel_space(lm_uv, W, H)
    pos = np.full((W * H, 3), np.uint32(0x7FC00000).view(f32), f32)
    nrm = np.zeros((W * H, 3), f32)
    i = np.flatnonzero(owner != NONE)
    if len(i) == 0:
        return pos, nrm
    t = owner[i].astype(np.int64)
    cx, cy = (i % W).astype(f32) + f32(0.5), (i // W).astype(f32) + f32(0.5)
    _, e1, e2, cover = edge_values(P[t], area[t], cx, cy)
    assert cover.all()
    wv, n, nm = shading_inputs(sd)
    with np.errstate(all="ignore"):
        bx, by = e1 / area[t], e2 / area[t]
        w = (f32(1.0) - bx) - by
        b = wv[t]
        pos[i] = np.stack([(b[:, k] * w + b[:, 3 + k] * bx) + b[:, 6 + k] * by for k in range(3)], 1)
        n0, n1, n2 = n[t, 0], n[t, 1], n[t, 2]
        v = (w[:, None] * n0 + bx[:, None] * n1) + by[:, None] * n2
        vx, vy, vz = _normalize(v[:, 0], v[:, 1], v[:, 2])
        m = nm[t]
        g = [(m[:, r] * vx + m[:, 3 + r] * vy) + m[:, 6 + r] * vz for r in range(3)]
        nrm[i] = np.stack(_normalize(*g), 1)
    assert pos.dtype == f32 and nrm.dtype == f32
    return pos, nrm


def entry_states(n_texels, repeats, seed):
    """Step 3: the state of entry e = i * repeats + k, (n_texels * repeats,) uint32"""
    e = np.arange(n_texels * repeats, dtype=np.uint64)
    s = (np.uint64(seed & 0xFFFFFFFF) + (e + np.uint64(1)) * np.uint64(0x9E3779B9)) % np.uint64(1 << 32)
    s[s == 0] = 0x9E3779B9
    return s.astype(np.uint32)


def resolve_model(owner, radiance, rays, repeats):
    """Step 5: (W * H, 4) float32 from the gather's outputs over the W * H * repeats entries (rays == NONE: rejected)"""
    n = len(owner)
    rad, rays = np.asarray(radiance, f32).reshape(n, repeats, 3), np.asarray(rays, np.uint32).reshape(n, repeats)
    sampled = (owner != NONE) & (rays != NONE).all(1)
    total = np.zeros((n, 3), f32)
    with np.errstate(all="ignore"):
        for k in range(repeats):
            total = total + rad[:, k]
        mean = total / f32(repeats)
    out = np.zeros((n, 4), f32)
    out[sampled, :3] = mean[sampled]
    out[sampled, 3] = 1.0
    return out


def dilate_model(rgba, passes):
    """Step 6 on a (H, W, 4) float32 plane"""
    cur = np.array(rgba, f32, copy=True)
    H, W = cur.shape[:2]
    for _ in range(passes):
        S, n = np.zeros((H, W, 3), f32), np.zeros((H, W), np.int64)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == 0 and dy == 0:
                    continue
                q = np.zeros_like(cur)  # the tap at (x + dx, y + dy); alpha 0 outside the atlas
                ys, yd = (slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0)))
                xs, xd = (slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0)))
                q[yd, xd] = cur[ys, xs]
                use = q[..., 3] > 0
                S = np.where(use[..., None], S + q[..., :3], S)
                n = n + use
        fill = (cur[..., 3] == 0) & (n > 0)
        nxt = cur.copy()
        with np.errstate(all="ignore"):
            nxt[fill, :3] = (S / np.maximum(n, 1).astype(f32)[..., None])[fill]
        nxt[fill, 3] = 0.5
        cur = nxt
    return cur


def stats_model(owner, rays, rgba, repeats):
    rays = np.asarray(rays, np.uint32).reshape(len(owner), repeats)
    a = rgba.reshape(-1, 4)[:, 3]
    return {"covered": int((owner != NONE).sum()), "sampled": int((a == 1.0).sum()), "filled": int((a == 0.5).sum()),
            "rays": int(rays[rays != NONE].astype(np.uint64).sum())}


# ---- UV sets the two files share ----------------------------------------------------------------------------------------------------------
def jittered_grid_uvs(W, H, seed, cells=8, lo=(3.2, 2.6), hi=(57.7, 44.1)):
    """A cells x cells grid of quads over the rectangle [lo, hi] (texels) of a W x H atlas: the inner vertices jittered by up to 0.35 of a
    cell, every quad split on one of its two diagonals, every triangle in one of the two windings, in a shuffled order. The triangles index
    one vertex array, so shared corners are bit-identical. -> (lm_uv (2 cells^2, 3, 2) float32, the rectangle in fp32 texel space)"""
    g = np.random.default_rng(seed)
    k = cells + 1
    step = np.array([(hi[0] - lo[0]) / cells, (hi[1] - lo[1]) / cells])
    v = np.stack(np.meshgrid(np.arange(k), np.arange(k), indexing="xy"), -1).astype(np.float64) * step + np.array(lo)
    v[1:-1, 1:-1] += g.uniform(-0.35, 0.35, size=(k - 2, k - 2, 2)) * step
    uv = (v / np.array([W, H])).astype(f32).reshape(-1, 2)
    tris = []
    for cy in range(cells):
        for cx in range(cells):
            a, b, c, d = cy * k + cx, cy * k + cx + 1, (cy + 1) * k + cx + 1, (cy + 1) * k + cx
            pair = [(a, b, c), (a, c, d)] if g.integers(2) else [(a, b, d), (b, c, d)]
            tris += [t if g.integers(2) else (t[0], t[2], t[1]) for t in pair]
    tris = np.array(tris)[g.permutation(len(tris))]
    P = uv.reshape(k, k, 2) * np.array([W, H], f32)
    rect = (P[0, 0, 0], P[0, 0, 1], P[-1, -1, 0], P[-1, -1, 1])
    assert (P[:, 0, 0] == rect[0]).all() and (P[:, -1, 0] == rect[2]).all() and (P[0, :, 1] == rect[1]).all() and (P[-1, :, 1] == rect[3]).all()
    return np.ascontiguousarray(uv[tris]), rect


def diagonal_quad_uvs(order):
    """The unit quad split on the diagonal (0, 0) -> (1, 1): on an 8 x 8 atlas it runs through the centres of the texels (k, k)"""
    a, b, c, d = (0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)
    t = [(a, b, c), (a, c, d)]
    return np.array([t[k] for k in order], f32)


# ---- the model alone ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_no_texel_centre_inside_a_mesh_of_shared_edges_is_left_empty(seed):
    W, H = 61, 47
    uv, (x0, y0, x1, y1) = jittered_grid_uvs(W, H, seed)
    owner = owner_model(uv, W, H, full=True)
    np.testing.assert_array_equal(owner, owner_model(uv, W, H))  # the boxes lose nothing
    cx, cy = np.arange(W, dtype=f32) + f32(0.5), np.arange(H, dtype=f32) + f32(0.5)
    inside = ((cy > y0) & (cy < y1))[:, None] & ((cx > x0) & (cx < x1))[None, :]
    assert inside.sum() > 2000
    covered = (owner != NONE).reshape(H, W)
    assert (covered & inside).sum() == inside.sum()  # zero holes
    outside = ((cy < y0) | (cy > y1))[:, None] | ((cx < x0) | (cx > x1))[None, :]
    assert not (covered & outside).any()
    assert len(np.unique(owner[owner != NONE])) > 100  # most of the 128 triangles hold a centre


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_texels_on_a_shared_diagonal_go_to_the_lower_index(order):
    owner = owner_model(diagonal_quad_uvs(order), 8, 8, full=True).reshape(8, 8)
    assert (owner != NONE).all()
    assert (np.diag(owner) == 0).all()
    lower = np.tril(np.ones((8, 8), bool), -1)  # y > x: the triangle (a, c, d)
    acd = order.index(1)
    assert (owner[lower] == acd).all() and (owner[lower.T] == 1 - acd).all()


def test_dilation_fills_one_ring_per_pass_and_keeps_every_texel_that_has_alpha():
    H, W = 11, 13
    g = np.random.default_rng(3)
    src = np.zeros((H, W, 4), f32)
    src[4:7, 5:8] = np.concatenate([g.uniform(0.1, 2.0, size=(3, 3, 3)), np.ones((3, 3, 1))], -1).astype(f32)
    src[0, 0] = (3.0, 5.0, 7.0, 1.0)
    yy, xx = np.mgrid[0:H, 0:W]
    dist = np.minimum(np.maximum(np.maximum(4 - yy, yy - 6), np.maximum(5 - xx, xx - 7)), np.maximum(yy, xx))  # Chebyshev, to either seed
    prev = src
    for p in range(1, 6):
        out = dilate_model(src, p)
        np.testing.assert_array_equal(out, dilate_model(prev, 1))  # p passes are one pass p times
        np.testing.assert_array_equal(out[..., 3] == 0.5, (dist >= 1) & (dist <= p))
        np.testing.assert_array_equal(out[..., 3] == 1.0, dist <= 0)
        keep = prev[..., 3] > 0
        np.testing.assert_array_equal(out[keep], prev[keep])
        prev = out
    one = dilate_model(src, 1)
    np.testing.assert_array_equal(one[1, 1], [3.0, 5.0, 7.0, 0.5])  # one tap: the mean of one
    np.testing.assert_array_equal(one[3, 6, :3], (f32(0) + src[4, 5, :3] + src[4, 6, :3] + src[4, 7, :3]) / f32(3.0))  # three taps, in tap order
    np.testing.assert_array_equal(one[3, 4, :3], src[4, 5, :3])
    np.testing.assert_array_equal(dilate_model(src, 0), src)


def test_entry_states_are_the_vertex_bakers_corner_seeds():
    for n, r, seed in ((35, 1, 0), (35, 3, 7), (1000, 2, 0xFFFFFFFF), (64 * 64, 3, 11)):
        np.testing.assert_array_equal(entry_states(n, r, seed), bake.corner_seeds(n, r, seed).reshape(-1))
    # the one state that would be 0: seed = -(e + 1) * 0x9E3779B9 for e = 4
    seed = (-(5 * 0x9E3779B9)) & 0xFFFFFFFF
    s = entry_states(8, 1, seed)
    assert s[4] == 0x9E3779B9 and (s != 0).all()


def test_resolve_model_means_in_order_and_drops_texels_with_a_rejected_entry():
    owner = np.array([0, NONE, 2, 5], np.uint32)
    rad = np.arange(24, dtype=f32).reshape(8, 3) + f32(0.1)
    rays = np.array([3, 4, NONE, NONE, 7, NONE, 1, 2], np.uint32)
    out = resolve_model(owner, rad, rays, 2)
    np.testing.assert_array_equal(out[0], np.append(((f32(0) + rad[0]) + rad[1]) / f32(2), f32(1)))
    np.testing.assert_array_equal(out[1:3], np.zeros((2, 4), f32))
    np.testing.assert_array_equal(out[3], np.append(((f32(0) + rad[6]) + rad[7]) / f32(2), f32(1)))
    assert stats_model(owner, rays, out, 2) == {"covered": 3, "sampled": 2, "filled": 0, "rays": 17}


@pytest.mark.parametrize("atlas", [a + (1,) for a in CORNELL_ATLASES] + [CORNELL_ORACLE_ATLAS])
def test_unwrap_gives_every_cornell_triangle_a_texel(atlas):
    sd = scenes.get_scene("cornell")
    W, H, gutter = atlas
    assert sd.n_triangles == 116
    uv = bake.triangle_grid_uvs(sd.n_triangles, W, H, gutter)
    assert uv.shape == (sd.n_triangles, 3, 2) and uv.dtype == f32 and (uv >= 0).all() and (uv <= 1).all()
    owner = owner_model(uv, W, H)
    assert len(np.unique(owner[owner != NONE])) == sd.n_triangles
    assert (owner == NONE).any()  # the gutters
    np.testing.assert_array_equal(owner, owner_model(uv, W, H, full=True))


def test_unwrap_refuses_cells_under_two_texels_inside_the_gutter():
    assert bake.triangle_grid_uvs(0, 8, 8).shape == (0, 3, 2)
    assert bake.triangle_grid_uvs(4, 8, 8).shape == (4, 3, 2)       # cells of 4, 2 inside the gutter
    assert bake.triangle_grid_uvs(16, 8, 8, gutter=0).shape == (16, 3, 2)
    for args in ((5, 8, 8), (17, 8, 8, 0), (1, 3, 9), (1, 64, 64, 32)):
        with pytest.raises(ValueError):
            bake.triangle_grid_uvs(*args)
    uv = bake.triangle_grid_uvs(7, 24, 12, gutter=2)  # cells of 6 (4 x 2 of them), 2 texels inside the gutter
    P = uv * np.array([24, 12], f32)
    assert np.array_equal(P, np.round(P)) and (P.max(1) - P.min(1) == 2).all()
    np.testing.assert_array_equal(P[4], [[2, 8], [4, 8], [2, 10]])  # triangle 4: the first cell of the second row


# ---- the library in front of the device ------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_prototyped(rtlib, devlib, tmp_path):
    """The test that fails without the feature: the seven names of the interface (six functions and the handle's type)."""
    header = (REPO / "include" / "rt_mi355x.h").read_text()
    assert "typedef struct rt_lightmap rt_lightmap;" in header
    for name in SYMBOLS:
        assert re.search(rf"^(int|void) +{name}\(", header, re.M), name
        assert name in abi.PROTOTYPES
        for lib in (rtlib, devlib):
            assert hasattr(lib, name), name
    assert rtlib.rt_abi_version() == 8 and "#define RT_ABI_VERSION 8" in header
    src = tmp_path / "layout.c"
    pf = [f[0] for f in abi.rt_lightmap_params._fields_]
    sf = [f[0] for f in abi.rt_lightmap_stats._fields_]
    assert pf == ["samples", "max_depth", "rr_start", "repeats", "seed", "dilate"] and sf == ["covered", "sampled", "filled", "reserved", "rays"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_mi355x.h"\nint main(void){' +
                   'printf("%zu %zu\\n", sizeof(rt_lightmap_params), sizeof(rt_lightmap_stats));' +
                   "".join(f'printf("%zu\\n", offsetof(rt_lightmap_params, {f}));' for f in pf) +
                   "".join(f'printf("%zu\\n", offsetof(rt_lightmap_stats, {f}));' for f in sf) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", str(REPO / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [24, 24] + [getattr(abi.rt_lightmap_params, f).offset for f in pf] + [getattr(abi.rt_lightmap_stats, f).offset for f in sf]
    assert got == want and C.sizeof(abi.rt_lightmap_params) == 24 and C.sizeof(abi.rt_lightmap_stats) == 24


def _err(lib):
    return lib.rt_last_error().decode()


def test_create_refuses_before_any_device_call(rtlib):
    """On a host-only scene no device call can succeed, so every status below was decided in front of the device: RT_ERR_INVALID with the
    cause named, and RT_ERR_NO_DEVICE only for a well-formed request."""
    sd = scenes.get_scene("cube")
    s = Scene(sd, device=-1)
    uv = bake.triangle_grid_uvs(sd.n_triangles, 64, 64).reshape(-1)
    h = C.c_void_p(0x1234)
    inv = abi.RT_ERR_INVALID

    def create(scene=s.h, w=64, hgt=64, r=1, lm_uv=abi.fptr(uv), out=C.byref(h)):
        return rtlib.rt_lightmap_create(scene, w, hgt, r, lm_uv, out)

    assert create(out=None) == inv and "null" in _err(rtlib)
    for kw, word in (({"scene": None}, "null scene"), ({"lm_uv": None}, "lm_uv"), ({"w": 0}, "1 .. 8192"), ({"hgt": 0}, "1 .. 8192"),
                     ({"w": -5}, "1 .. 8192"), ({"w": 8193}, "1 .. 8192"), ({"hgt": 8193}, "1 .. 8192"), ({"r": 0}, "max_repeats"),
                     ({"w": 8192, "hgt": 8192, "r": 32}, "2^31"), ({"w": 1024, "hgt": 1024, "r": 2048}, "2^31"),
                     ({"r": 0xFFFFFFFF}, "2^31")):
        h.value = 0x1234
        assert create(**kw) == inv, kw
        assert word in _err(rtlib), (kw, _err(rtlib))
        assert not h.value  # the output is cleared
    for kw in ({}, {"w": 1, "hgt": 1}, {"w": 8192, "hgt": 8192, "r": 31}, {"w": 7, "hgt": 5, "r": 3}):
        assert create(**kw) == abi.RT_ERR_NO_DEVICE, kw
        assert "host-only" in _err(rtlib) and not h.value
    e = Scene(scenes.get_scene("empty"), device=-1)
    assert create(scene=e.h, lm_uv=None) == abi.RT_ERR_NO_DEVICE  # no triangle: no UV is required
    rtlib.rt_lightmap_destroy(None)
    e.close(), s.close()


def test_calls_refuse_null_handles_and_bad_parameters_before_any_device_call(rtlib):
    """No lightmap exists without a device, so the handle is NULL throughout: the parameters are checked in front of it, each cause named."""
    inv = abi.RT_ERR_INVALID
    buf = np.zeros(16, f32)
    tri = np.zeros(4, np.uint32)
    st = abi.rt_lightmap_stats()

    def params(samples=4, max_depth=5, rr_start=0, repeats=1, seed=1, dilate=0):
        return abi.rt_lightmap_params(samples, max_depth, rr_start, repeats, seed, dilate)

    assert rtlib.rt_lightmap_texels(None, abi.u32ptr(tri), abi.fptr(buf), abi.fptr(buf)) == inv and "null" in _err(rtlib)
    assert rtlib.rt_lightmap_texels_device(None, None, None, None, None) == inv and "null" in _err(rtlib)
    for call in (lambda p: rtlib.rt_lightmap_bake(None, p, abi.fptr(buf), C.byref(st)),
                 lambda p: rtlib.rt_lightmap_bake_device(None, p, None, None, None)):
        assert call(None) == inv and "null parameters" in _err(rtlib)
        for kw, word in (({"samples": 0}, "samples"), ({"max_depth": 0}, "max_depth"), ({"repeats": 0}, "repeats"), ({"dilate": 17}, "dilate"),
                         ({"dilate": 0xFFFFFFFF}, "dilate")):
            assert call(C.byref(params(**kw))) == inv, kw
            assert word in _err(rtlib), (kw, _err(rtlib))
        for kw in ({}, {"dilate": 16}, {"rr_start": 3, "repeats": 1000}):
            assert call(C.byref(params(**kw))) == inv and "null argument" in _err(rtlib)


def test_python_wrappers_refuse_wrong_shapes(rtlib):
    sd = scenes.get_scene("cube")
    s = Scene(sd, device=-1)
    t = sd.n_triangles
    uv = bake.triangle_grid_uvs(t, 64, 64)
    for good in (uv, uv.reshape(t, 6), uv.astype(np.float64)):
        with pytest.raises(abi.RtError) as e:
            Lightmap(s, good, 64, 64)
        assert e.value.status == abi.RT_ERR_NO_DEVICE
    for bad in (uv[:-1], uv.reshape(-1), uv.reshape(t, 2, 3), np.zeros((t, 3, 3), f32), np.zeros((t, 6), np.int32), uv.reshape(t * 3, 2)):
        with pytest.raises(ValueError):
            Lightmap(s, bad, 64, 64)
    for kw in ({"width": 0, "height": 64}, {"width": 64, "height": 8193}, {"width": 64, "height": 64, "max_repeats": 0}):
        with pytest.raises(abi.RtError) as e:
            Lightmap(s, uv, **kw)
        assert e.value.status == abi.RT_ERR_INVALID
    s.close()
