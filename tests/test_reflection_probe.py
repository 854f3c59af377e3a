"""Reflection probes (include/rt_mi355x.h: rt_reflection_probes_*) without a GPU: the numpy model of the contract's steps 1 and 3 to 6 that
tests/test_gpu_reflection_probe.py compares the device with (face_dir_model, entries_model, resolve_model, table_model, prefilter_model,
sample_model, and bake_model, the whole bake around a path tracer handed in), what the model itself must show (the cube's table and its
inverse, the table's solid angles, the empty scene through the CPU oracle, the constant chain, the lobe of one bright texel, the parallax
box), and the library in front of the device: the exported symbols, the struct layouts, the refusals in their order, the wrappers' shape
checks. The refusals that need an object (spt, max_depth, clamp, calls before a level 0, stale levels) cannot be reached without a device:
tests/test_gpu_reflection_probe.py has them."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rtamd import abi, bake, scenes
from rtamd.renderer import ReflectionProbes, Scene
from test_lightmap import entry_states
from test_path_query import xorshift_model
from test_probe_volume import contract_range_model

REPO = Path(__file__).resolve().parent.parent
f32 = np.float32
NONE = 0xFFFFFFFF
SYMBOLS = ["rt_reflection_probes_create", "rt_reflection_probes_destroy", "rt_reflection_probes_entries", "rt_reflection_probes_entries_device",
           "rt_reflection_probes_bake", "rt_reflection_probes_bake_device", "rt_reflection_probes_set_level0",
           "rt_reflection_probes_set_level0_device", "rt_reflection_probes_prefilter", "rt_reflection_probes_prefilter_device",
           "rt_reflection_probes_get_chain", "rt_reflection_probes_get_chain_device", "rt_reflection_probes_sample",
           "rt_reflection_probes_sample_device"]
ONE, TWO, HALF = f32(1.0), f32(2.0), f32(0.5)


# ---- the model both files share ---------------------------------------------------------------------------------------------------------
def chain_texels(size, levels):
    return sum(6 * (size >> l) ** 2 for l in range(levels))


def level_offset(size, l):
    return sum(6 * (size >> m) ** 2 for m in range(l))


def face_dir_model(f, s, t):
    """The cube's table: the unnormalised direction of face f at (s, t), arrays -> (n, 3) float32"""
    f, s, t = np.asarray(f), np.asarray(s, f32), np.asarray(t, f32)
    one = np.ones_like(s)
    rows = [(one, -t, -s), (-one, -t, s), (s, one, t), (s, -one, -t), (s, -t, one), (-s, -t, -one)]
    d = np.zeros(s.shape + (3,), f32)
    for k, row in enumerate(rows):
        d = np.where((f == k)[..., None], np.stack(row, -1), d)
    assert d.dtype == f32
    return d


def centre_model(x, S):
    """s of texel x's centre at a level of S texels on an edge"""
    return (np.asarray(x).astype(f32) + HALF) * (TWO / f32(S)) - ONE


def unit_model(v):
    """unit(v): (v * i (n, 3), (i * i) * i), i = 1 / sqrt(dot(v, v)), the dot in v's component order"""
    v = np.asarray(v, f32)
    i = ONE / np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    assert i.dtype == f32
    return v * i[..., None], (i * i) * i


def level_dirs_model(S):
    """unit() of the centre directions of a level's 6 * S * S texels in layout order -> (d (n, 3), o (n,))"""
    f, y, x = np.meshgrid(np.arange(6), np.arange(S), np.arange(S), indexing="ij")
    return unit_model(face_dir_model(f.reshape(-1), centre_model(x.reshape(-1), S), centre_model(y.reshape(-1), S)))


def table_model(size):
    """Step 4's table: (6 * size^2, 4) float32, (d_k, o_k)"""
    d, o = level_dirs_model(size)
    return np.concatenate([d, o[:, None]], 1)


def entries_model(positions, size, spt, seed):
    """Step 1: {"pos", "dir": (entries, 3) float32, "state": (entries,) uint32, the path states, "state0": the states before the two draws}"""
    positions = np.asarray(positions, f32).reshape(-1, 3)
    count = len(positions)
    n_tex = count * 6 * size * size
    a0 = entry_states(n_tex, spt, seed)
    u1, a1 = xorshift_model(a0)
    u2, a2 = xorshift_model(a1)
    T = np.arange(n_tex * spt) // spt
    x, y, f, p = T % size, (T // size) % size, (T // (size * size)) % 6, T // (6 * size * size)
    step = TWO / f32(size)
    s = (x.astype(f32) + u1) * step - ONE
    t = (y.astype(f32) + u2) * step - ONE
    assert s.dtype == f32 and u1.dtype == f32
    return {"pos": positions[p], "dir": face_dir_model(f, s, t), "state": a2, "state0": a0}


def resolve_model(radiance, rays, count, size, spt, clamp):
    """Steps 3 and 5 from the path query's outputs over the entries (rays == NONE: rejected) -> (level 0 (count, 6 * size^2, 4), stats)"""
    K = 6 * size * size
    rad = np.asarray(radiance, f32).reshape(count, K, spt, 3)
    rays = np.asarray(rays, np.uint32).reshape(count, K, spt)
    valid = rays[:, 0, 0] != NONE
    lv = np.zeros((count, K, 4), f32)
    with np.errstate(all="ignore"):
        c = np.zeros((count, K, 3), f32)
        for j in range(spt):
            r = rad[:, :, j]
            if clamp > 0:
                r = np.fmin(r, f32(clamp))
            c = c + r
        lv[:, :, :3] = c / f32(spt)
    lv[:, :, 3] = 1.0
    lv[~valid] = 0.0
    assert lv.dtype == f32
    return lv, {"probes": count, "valid": int(valid.sum()), "rays": int(rays[valid].astype(np.uint64).sum())}


def prefilter_model(level0, size, levels):
    """Step 4: the chain (count, chain_texels, 4) float32 from level 0 (count, 6 * size^2, 4). A Python loop over the level-0 texels,
    vectorised over the outputs and the probes in float32: the order of the additions is the contract's."""
    level0 = np.asarray(level0, f32).reshape(-1, 6 * size * size, 4)
    count, K = level0.shape[:2]
    valid = level0[:, 0, 3] != 0
    chain = np.zeros((count, chain_texels(size, levels), 4), f32)
    chain[:, :K] = level0
    tab = table_model(size)
    with np.errstate(all="ignore"):
        for l in range(1, levels):
            n, _ = level_dirs_model(size >> l)
            M, q = len(n), 2 * (levels - l) - 1
            W, A = np.zeros(M, f32), np.zeros((count, M, 3), f32)
            for k in range(K):
                c = (n[:, 0] * tab[k, 0] + n[:, 1] * tab[k, 1]) + n[:, 2] * tab[k, 2]
                on = c > 0
                w = c
                for _ in range(q):
                    w = w * w
                w = w * tab[k, 3]
                W = np.where(on, W + w, W)
                A = np.where(on[None, :, None], A + w[None, :, None] * level0[:, k, None, :3], A)
            o = level_offset(size, l)
            chain[:, o:o + M, :3] = A / W[None, :, None]
            chain[:, o:o + M, 3] = 1.0
            assert W.dtype == f32 and A.dtype == f32
    chain[~valid, K:] = 0.0
    return chain


def prefilter_outputs_model(level0, size, levels, l, outs):
    """Step 4 for the outputs `outs` of level l of ONE probe whose level 0 (6 * size^2, 4) is finite -> (len(outs), 4): for the sizes at
    which prefilter_model's loop is too slow. A sum that started at +0 does not change a bit when +-0 is added to it, and a weight of 0 times
    a finite texel is +-0, so for finite texels the skipped term is a term of weight 0 and the ordered sum is the last column of
    np.add.accumulate, which adds strictly in order (test_the_accumulated_prefilter_is_the_loop holds the two together)."""
    level0 = np.asarray(level0, f32).reshape(6 * size * size, 4)
    assert np.isfinite(level0).all() and level0[0, 3] != 0
    tab = table_model(size)
    n = level_dirs_model(size >> l)[0][np.asarray(outs)]
    c = (n[:, 0, None] * tab[None, :, 0] + n[:, 1, None] * tab[None, :, 1]) + n[:, 2, None] * tab[None, :, 2]
    w = c
    for _ in range(2 * (levels - l) - 1):
        w = w * w
    w = np.where(c > 0, w * tab[None, :, 3], f32(0.0))
    W = np.add.accumulate(w, axis=1)[:, -1]
    out = np.ones((len(n), 4), f32)
    for ch in range(3):
        out[:, ch] = np.add.accumulate(w * level0[None, :, ch], axis=1)[:, -1] / W
    assert w.dtype == f32 and W.dtype == f32
    return out


def lookup_dir_model(centres, boxes, idx, pos, dirs):
    """Step 6 up to the lookup direction: (L (n, 3) float32, ok (n,) bool: not one of the inputs that give NaNs so far)"""
    centres = np.asarray(centres, f32).reshape(-1, 3)
    idx, r = np.asarray(idx).astype(np.int64), np.array(dirs, f32, copy=True)
    ok = (idx >= 0) & (idx < len(centres)) & np.isfinite(r).all(1)
    if pos is not None:
        q = np.asarray(pos, f32)
        ok &= np.isfinite(q).all(1)
    p = np.where(ok, idx, 0)
    if pos is not None and boxes is not None:
        b = np.asarray(boxes, f32).reshape(-1, 6)[p]
        with np.errstate(all="ignore"):
            ta = [np.where(r[:, a] == 0, f32(np.inf), (np.where(r[:, a] > 0, b[:, 3 + a], b[:, a]) - q[:, a]) / r[:, a]) for a in range(3)]
            t = np.fmin(np.fmin(ta[0], ta[1]), ta[2])
            L = (q + r * t[:, None]) - centres[p]
        assert t.dtype == f32 and L.dtype == f32
        use = ok & (t > 0) & np.isfinite(t)
        r = np.where(use[:, None], L, r)
        ok &= ~use | np.isfinite(L).all(1)
    return r, ok


def face_st_model(L):
    """The inverse of the cube's table: (face, s, t, m) of directions L (n, 3), m the major |component|"""
    L = np.asarray(L, f32)
    ax, ay, az = np.abs(L[:, 0]), np.abs(L[:, 1]), np.abs(L[:, 2])
    axis = np.where((ax >= ay) & (ax >= az), 0, np.where(ay >= az, 1, 2))
    m = np.where(axis == 0, ax, np.where(axis == 1, ay, az))
    pos = np.where(axis == 0, L[:, 0], np.where(axis == 1, L[:, 1], L[:, 2])) > 0
    f = 2 * axis + np.where(pos, 0, 1)
    x, y, z = L[:, 0], L[:, 1], L[:, 2]
    with np.errstate(all="ignore"):
        s = np.select([f == 0, f == 1, f == 5], [-z, z, -x], x) / m
        t = np.select([f == 2, f == 3], [z, -z], -y) / m
    assert s.dtype == f32 and t.dtype == f32
    return f, s, t, m


def bilinear_model(lvl, S, p, f, s, t):
    """One level of step 6: lvl (count, 6, S, S, 4), per point its probe p, face f and (s, t) -> (n, 3)"""
    def axis(u):
        g = np.fmin(np.fmax((u + ONE) * (HALF * f32(S)) - HALF, f32(0.0)), f32(S - 1))
        i0 = np.minimum(g.astype(np.int64), S - 2)
        fr = g - i0.astype(f32)
        return i0, (ONE - fr, fr)
    x0, wx = axis(s)
    y0, wy = axis(t)
    acc = np.zeros((len(p), 3), f32)
    for dy in range(2):
        for dx in range(2):
            acc = acc + (wy[dy] * wx[dx])[:, None] * lvl[p, f, y0 + dy, x0 + dx, :3]
    assert acc.dtype == f32
    return acc


def sample_model(chain, size, levels, centres, boxes, idx, pos, dirs, lod):
    """Step 6: (n, 3) float32"""
    chain = np.asarray(chain, f32)
    count = chain.shape[0]
    lod = np.asarray(lod, f32)
    L, ok = lookup_dir_model(centres, boxes, idx, pos, dirs)
    ok &= np.isfinite(lod)
    f, s, t, m = face_st_model(np.where(ok[:, None], L, f32(1.0)))
    ok &= m > 0
    p =np.where(ok, np.asarray(idx).astype(np.int64), 0)
    s, t = np.where(ok, s, f32(0.0)), np.where(ok, t, f32(0.0))
    ld = np.fmin(np.fmax(np.where(ok, lod, f32(0.0)), f32(0.0)), f32(levels - 1))
    with np.errstate(all="ignore"):
        per_level = [bilinear_model(chain[:, level_offset(size, l):level_offset(size, l + 1)].reshape(count, 6, size >> l, size >> l, 4),
                                    size >> l, p, f, s, t) for l in range(levels)]
        if levels == 1:
            out = per_level[0]
        else:
            l0 = np.minimum(ld.astype(np.int64), levels - 2)
            fl = ld - l0.astype(f32)
            stack = np.stack(per_level, 0)
            a, b = stack[l0, np.arange(len(p))], stack[l0 + 1, np.arange(len(p))]
            out = a * (ONE - fl)[:, None] + b * fl[:, None]
    out = np.where((chain[p, 0, 3] == 0)[:, None], f32(0.0), out)
    out = np.where(ok[:, None], out, f32(np.nan))
    assert out.dtype == f32
    return out


def bake_model(trace, sd, positions, size, levels, spt, max_depth, rr_start, seed, clamp=0.0):
    """The bake as the contract states it: the model's entries, `trace` (OracleScene.trace_paths or Scene.trace_paths) over the entries of
    the probes inside the contract range, the model's resolve and prefilter -> (chain (count, chain_texels, 4), stats)"""
    positions = np.asarray(positions, f32).reshape(-1, 3)
    e = entries_model(positions, size, spt, seed)
    n = len(e["pos"])
    ok = contract_range_model(sd)(e["pos"])
    rad, rays = np.full((n, 3), np.nan, f32), np.full(n, NONE, np.uint32)
    if ok.any():
        out = trace(e["pos"][ok], e["dir"][ok], e["state"][ok], max_depth, samples=1, rr_start=rr_start)
        rad[ok], rays[ok] = out["radiance"], out["rays"]
    lv, stats = resolve_model(rad, rays, len(positions), size, spt, clamp)
    return prefilter_model(lv, size, levels), stats


def zero_state_seed():
    """The seed under which entry 0's raw state, seed + 0x9E3779B9, is 0 and is replaced: found by walking the 2^32 seeds from the one
    the rule's inverse names (the search ends at its first step; it is a search so that a change of the rule shows here)"""
    start = (-0x9E3779B9) & 0xFFFFFFFF
    for seed in range(start, start + 4):
        if (seed + 0x9E3779B9) & 0xFFFFFFFF == 0:
            assert entry_states(4, 1, seed)[0] == 0x9E3779B9
            return seed
    raise AssertionError("no seed makes entry 0's state zero")


def smooth_level0(count, size, seed, invalid=()):
    """A synthetic level 0 (count, 6, size, size, 4): positive random values, validity 1, the `invalid` probes zero"""
    g = np.random.default_rng(seed)
    lv = np.zeros((count, 6, size, size, 4), f32)
    lv[..., :3] = g.uniform(0.1, 3.0, size=(count, 6, size, size, 3))
    lv[..., 3] = 1.0
    lv[list(invalid)] = 0.0
    return lv


# ---- the model alone ----------------------------------------------------------------------------------------------------------------------
def test_texel_centres_map_back_to_their_face_and_texel():
    S = 8
    f, y, x = (a.reshape(-1) for a in np.meshgrid(np.arange(6), np.arange(S), np.arange(S), indexing="ij"))
    d = face_dir_model(f, centre_model(x, S), centre_model(y, S))
    for v in (d, unit_model(d)[0], d * f32(37.5)):  # any length
        ff, s, t, m = face_st_model(v)
        np.testing.assert_array_equal(ff, f)
        np.testing.assert_array_equal(np.floor((s.astype(np.float64) + 1) * 0.5 * S).astype(int), x)
        np.testing.assert_array_equal(np.floor((t.astype(np.float64) + 1) * 0.5 * S).astype(int), y)
        assert (m > 0).all()
    # the six axes are the faces' centres
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f32)
    ff, s, t, _ = face_st_model(axes)
    np.testing.assert_array_equal(ff, np.arange(6))
    assert (s == 0).all() and (t == 0).all()
    np.testing.assert_array_equal(face_dir_model(np.arange(6), np.zeros(6, f32), np.zeros(6, f32)), axes)


def test_directions_on_face_diagonals_take_the_stated_tie():
    L = np.array([[1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 1], [-1, -1, -1], [0, -1, 1], [-1, 1, 0.5], [0.5, -1, -1], [-2, 0, 2], [0, 3, -3]], f32)
    ff = face_st_model(L)[0]
    np.testing.assert_array_equal(ff, [0, 0, 2, 0, 1, 3, 1, 3, 1, 2])  # x before y before z


def test_table_weights_sum_to_the_sphere():
    size = 32
    tab = table_model(size)
    assert tab.shape == (6 * size * size, 4) and tab.dtype == f32
    want = 4.0 * np.pi / (2.0 / size) ** 2
    assert abs(tab[:, 3].astype(np.float64).sum() - want) <= 1e-3 * want
    np.testing.assert_allclose(np.linalg.norm(tab[:, :3].astype(np.float64), axis=1), 1.0, atol=4 * 2.0 ** -23)


def test_entries_model_layout_and_the_replaced_zero_state():
    pos = np.array([[1.0, 2.0, 3.0], [-4.0, 0.5, 0.25]], f32)
    seed = zero_state_seed()
    e = entries_model(pos, 8, 3, seed)
    n = 2 * 6 * 64 * 3
    assert e["pos"].shape == (n, 3) and e["dir"].shape == (n, 3) and e["state"].shape == (n,)
    assert e["state0"][0] == 0x9E3779B9 and (e["state0"] != 0).all()
    np.testing.assert_array_equal(e["pos"][:n // 2], np.broadcast_to(pos[0], (n // 2, 3)))
    np.testing.assert_array_equal(e["pos"][n // 2:], np.broadcast_to(pos[1], (n // 2, 3)))
    # every entry's direction lies inside its own texel of its own face
    T = np.arange(n) // 3
    f, s, t, _ = face_st_model(e["dir"])
    np.testing.assert_array_equal(f, (T // 64) % 6)
    fx, fy = (s.astype(np.float64) + 1) * 4, (t.astype(np.float64) + 1) * 4
    assert ((fx >= T % 8 - 1e-6) & (fx <= T % 8 + 1 + 1e-6)).all() and ((fy >= (T // 8) % 8 - 1e-6) & (fy <= (T // 8) % 8 + 1 + 1e-6)).all()
    # two draws per entry
    np.testing.assert_array_equal(e["state"], xorshift_model(xorshift_model(e["state0"])[1])[1])


def test_empty_scene_through_the_oracle_gives_the_sky_at_every_level(oracle):
    sd = scenes.get_scene("empty")
    osc = oracle.OracleScene(sd)
    sky = np.asarray(sd.sky, f32)
    assert (sky > 0).any()
    pos = np.array([[0.0, 1.0, -2.0], [3.0, 0.0, 0.5]], f32)
    for size, levels, spt in ((8, 2, 1), (8, 2, 2), (16, 3, 1)):
        chain, stats = bake_model(osc.trace_paths, sd, pos, size, levels, spt, 5, 0, 3)
        K = 6 * size * size
        assert stats == {"probes": 2, "valid": 2, "rays": 2 * K * spt}
        assert chain.shape == (2, chain_texels(size, levels), 4) and (chain[..., 3] == 1).all()
        np.testing.assert_array_equal(chain[:, :K, :3], np.broadcast_to(sky, (2, K, 3)))  # level 0 is the sky exactly
        # a higher texel is a ratio of two sequential sums of K non-negative terms with the same weights: K * 2^-23 relative
        err = np.abs(chain[:, K:, :3].astype(np.float64) - sky.astype(np.float64))
        assert (err <= K * 2.0 ** -23 * sky.astype(np.float64)).all(), err.max()


def test_a_constant_chain_samples_to_its_value_at_any_direction_and_lod():
    g = np.random.default_rng(1)
    size, levels = 16, 3
    Lc = np.array([0.7, 1.3, 0.02], f32)
    chain = np.zeros((2, chain_texels(size, levels), 4), f32)
    chain[..., :3], chain[..., 3] = Lc, 1.0
    n = 500
    d = g.normal(size=(n, 3)).astype(f32) * f32(3.0)
    lod = g.uniform(-1.0, levels, size=n).astype(f32)
    idx = g.integers(0, 2, n)
    centres = np.array([[0, 0, 0], [1, 2, 3]], f32)
    boxes = np.array([[-1, -1, -1, 1, 1, 1], [0, 0, 0, 2, 4, 6]], f32)
    pos = g.uniform(-2, 5, size=(n, 3)).astype(f32)  # inside and outside the boxes
    for args in ((None, None), (boxes, pos), (None, pos), (boxes, None)):
        out = sample_model(chain, size, levels, centres, args[0], idx, args[1], d, lod)
        np.testing.assert_allclose(out, np.broadcast_to(Lc, out.shape), rtol=1e-6)
    one = np.zeros((1, chain_texels(size, 1), 4), f32)
    one[..., :3], one[..., 3] = Lc, 1.0
    np.testing.assert_allclose(sample_model(one, size, 1, centres[:1], None, np.zeros(n, int), None, d, lod), np.broadcast_to(Lc, (n, 3)), rtol=1e-6)


def test_sample_model_edges():
    size, levels = 8, 2
    chain = prefilter_model(smooth_level0(2, size, 3, invalid=(1,)), size, levels)
    assert (chain[1] == 0).all() and (chain[0, :, 3] == 1).all()
    centres = np.zeros((2, 3), f32)
    nan, inf = np.nan, np.inf
    d = np.array([[1, 0, 0], [0, 0, 0], [nan, 0, 1], [0, inf, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0], [1, 2, 3]], f32)
    idx = np.array([0, 0, 0, 0, 2, 1, 0, 0])
    lod = np.array([0, 0, 0, 0, 0, 0, nan, 0.5], f32)
    out = sample_model(chain, size, levels, centres, None, idx, None, d, lod)
    assert np.isfinite(out[0]).all() and np.isnan(out[[1, 2, 3, 4, 6]]).all() and (out[5] == 0).all() and np.isfinite(out[7]).all()
    # a direction through a texel centre at lod 0 is within a rounding of that texel (the bilinear weights are (1, 0) up to an ulp of s)
    lv0 = chain[0, :6 * 64].reshape(6, 8, 8, 4)
    c = face_dir_model(np.array([3]), centre_model(np.array([5]), 8), centre_model(np.array([2]), 8))
    got = sample_model(chain, size, levels, centres, None, [0], None, c, [0.0])
    np.testing.assert_allclose(got[0], lv0[3, 2, 5, :3], rtol=1e-5)
    # lod beyond both ends is the end
    np.testing.assert_array_equal(sample_model(chain, size, levels, centres, None, [0, 0], None, np.tile(d[7:], (2, 1)), [-3.0, 9.0]),
                                  sample_model(chain, size, levels, centres, None, [0, 0], None, np.tile(d[7:], (2, 1)), [0.0, 1.0]))


def test_one_bright_texel_gives_the_cosine_power_lobe_at_every_level():
    size, levels = 8, 3  # (the model takes a chain the library would refuse at this size: the lobes are what is looked at, two of them)
    K = 6 * size * size
    tab = table_model(size).astype(np.float64)
    for k0 in (0, 200, K - 1):
        lv = np.zeros((1, K, 4), f32)
        lv[0, :, 3] = 1.0
        lv[0, k0, :3] = (1.0, 2.0, 0.5)
        chain = prefilter_model(lv, size, levels)
        for l in range(1, levels):
            S = size >> l
            n = level_dirs_model(S)[0].astype(np.float64)
            q = 2 * (levels - l) - 1
            cos = n @ tab[:, :3].T                                   # (M, K)
            W = (np.maximum(cos, 0.0) ** (2 ** q) * tab[None, :, 3]).sum(1)
            want = np.maximum(cos[:, k0], 0.0) ** (2 ** q) * tab[k0, 3] / W
            got = chain[0, level_offset(size, l):level_offset(size, l + 1), 0].astype(np.float64)
            np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-30)
            np.testing.assert_allclose(chain[0, level_offset(size, l):level_offset(size, l + 1), 1], 2 * got, rtol=1e-6, atol=1e-30)
            assert (got[cos[:, k0] <= 0] == 0).all()                 # nothing behind the lobe
            order = np.argsort(cos[:, k0])
            lobe = (got * W)[order]                                   # monotone in the angle
            assert (lobe[1:] >= lobe[:-1] * (1 - 1e-4)).all()
            assert got.max() > 0


def test_a_non_finite_texel_behind_the_lobe_does_not_reach_the_sum():
    size, levels = 8, 2
    lv = smooth_level0(1, size, 5).reshape(1, -1, 4)
    k0 = 6 * 64 - 1  # face 5, the -z axis' corner texel
    clean = prefilter_model(lv, size, levels)
    lv[0, k0, :3] = np.inf
    dirty = prefilter_model(lv, size, levels)
    n = level_dirs_model(4)[0]
    behind = ~((n[:, 0] * table_model(8)[k0, 0] + n[:, 1] * table_model(8)[k0, 1]) + n[:, 2] * table_model(8)[k0, 2] > 0)
    assert behind.any() and not behind.all()
    o = level_offset(size, 1)
    np.testing.assert_array_equal(dirty[0, o:][behind], clean[0, o:][behind])
    assert not np.isfinite(dirty[0, o:][~behind, :3]).any()


def test_the_accumulated_prefilter_is_the_loop():
    for size, levels in ((8, 2), (16, 3)):
        lv = smooth_level0(1, size, 12).reshape(-1, 4)
        lv[7, :3] = 1e30
        lv[11, 1] = -2.5  # a negative texel: its skipped term is -0
        chain = prefilter_model(lv[None], size, levels)[0]
        for l in range(1, levels):
            M = 6 * (size >> l) ** 2
            got = prefilter_outputs_model(lv, size, levels, l, np.arange(M))
            np.testing.assert_array_equal(got.view(np.uint32), chain[level_offset(size, l):level_offset(size, l) + M].view(np.uint32))


def test_the_parallax_box():
    g = np.random.default_rng(7)
    n = 300
    r = g.normal(size=(n, 3)).astype(f32)
    centres = np.array([[0.5, 0.5, 0.5]], f32)
    boxes = np.array([[0, 0, 0, 1, 1, 1]], f32)
    idx = np.zeros(n, int)
    # at the centre the lookup direction is r up to its length
    L, ok = lookup_dir_model(centres, boxes, idx, np.broadcast_to(centres[0], (n, 3)), r)
    assert ok.all()
    unit = lambda v: v.astype(np.float64) / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)
    np.testing.assert_allclose(unit(L), unit(r), atol=1e-6)
    # off-centre in the unit box: the point where the ray leaves the box, seen from the centre, against float64
    pos = g.uniform(0.05, 0.95, size=(n, 3)).astype(f32)
    L, ok = lookup_dir_model(centres, boxes, idx, pos, r)
    assert ok.all()
    p64, r64 = pos.astype(np.float64), r.astype(np.float64)
    t64 = np.min(np.where(r64 > 0, (1 - p64) / r64, np.where(r64 < 0, (0 - p64) / r64, np.inf)), axis=1)
    want = p64 + r64 * t64[:, None] - 0.5
    np.testing.assert_allclose(L, want, atol=1e-5)
    assert np.abs(np.abs(want).max(1) - 0.5).max() < 1e-12  # (the hit lies on the box)
    # outside the box behind every slab (t <= 0), without pos and without boxes: r unchanged
    far = np.array([[2.0, 0.5, 0.5]], f32)
    np.testing.assert_array_equal(lookup_dir_model(centres, boxes, [0], far, np.array([[1.0, 0, 0]], f32))[0], [[1.0, 0, 0]])
    np.testing.assert_array_equal(lookup_dir_model(centres, boxes, idx, None, r)[0], r)
    np.testing.assert_array_equal(lookup_dir_model(centres, None, idx, pos, r)[0], r)


def test_the_python_helpers():
    lod = bake.lod_for_roughness(5, [0.0, 1.0, 2.0, 0.5])
    assert lod.dtype == f32 and lod[0] == 0 and lod[1] == 4 and lod[2] == 4 and 0 < lod[3] < 4
    for levels in (1, 3, 6):  # the roughness whose Phong exponent is level l's power maps to l
        for l in range(1, levels):
            a = np.sqrt(2.0 / (2.0 ** (2 * (levels - l) - 1) + 2.0))
            assert abs(float(bake.lod_for_roughness(levels, a)) - l) < 1e-5
        assert (np.diff(bake.lod_for_roughness(levels, np.linspace(0, 1, 50))) >= 0).all()
    with pytest.raises(ValueError):
        bake.lod_for_roughness(0, 0.5)
    v, n = np.array([[1, -1, 0], [0, 0, -1]], f32), np.array([[0, 1, 0], [0, 0, 1]], f32)
    np.testing.assert_array_equal(bake.reflect_dirs(v, n), [[1, 1, 0], [0, 0, 1]])
    with pytest.raises(ValueError):
        bake.reflect_dirs(v, n[:1])


# ---- the library in front of the device ------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_prototyped(rtlib, devlib, tmp_path):
    """The test that fails without the feature: the fifteen names of the interface (fourteen functions and the handle's type)."""
    header = (REPO / "include" / "rt_mi355x.h").read_text()
    assert "typedef struct rt_reflection_probes rt_reflection_probes;" in header
    for name in SYMBOLS:
        assert re.search(rf"^(int|void) +{name}\(", header, re.M), name
        assert name in abi.PROTOTYPES
        for lib in (rtlib, devlib):
            assert hasattr(lib, name), name
    assert rtlib.rt_abi_version() == 8 and "#define RT_ABI_VERSION 8" in header
    structs = {"rt_reflection_probes_desc": (32, ["count", "size", "levels", "max_spt", "pos", "box"]),
               "rt_reflection_bake_params": (20, ["spt", "max_depth", "rr_start", "seed", "clamp"]),
               "rt_reflection_stats": (16, ["probes", "valid", "rays"])}
    src = tmp_path / "layout.c"
    body, want = "", []
    for name, (size, fields) in structs.items():
        ct = getattr(abi, name)
        assert [f[0] for f in ct._fields_] == fields and C.sizeof(ct) == size
        body += f'printf("%zu\\n", sizeof({name}));' + "".join(f'printf("%zu\\n", offsetof({name}, {f}));' for f in fields)
        want += [size] + [getattr(ct, f).offset for f in fields]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_mi355x.h"\nint main(void){' + body + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", str(REPO / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want


def _err(lib):
    return lib.rt_last_error().decode()


_POS = np.zeros(3 * 4096, f32)
_BOX = np.tile(np.array([-1, -1, -1, 1, 1, 1], f32), 4096)


def _desc(count=2, size=8, levels=2, max_spt=4, pos=_POS, box=None):
    return abi.rt_reflection_probes_desc(count, size, levels, max_spt, abi.fptr(pos) if pos is not None else None,
                                         abi.fptr(box) if box is not None else None)


def test_create_refuses_in_the_stated_order_before_any_device_call(rtlib):
    """On a host-only scene no device call can succeed, so every status below was decided in front of the device: RT_ERR_INVALID with the
    cause named, and RT_ERR_NO_DEVICE only for a well-formed request. Each request carries the faults of every later step too (as far as
    they can stand together), so the word in the message shows which check came first."""
    s = Scene(scenes.get_scene("cube"), device=-1)
    h = C.c_void_p(0x1234)
    inv, nan, inf = abi.RT_ERR_INVALID, float("nan"), float("inf")
    bad_pos = _POS.copy()
    bad_pos[4] = nan
    bad_box = _BOX.copy()
    bad_box[6 + 1], bad_box[6 + 4] = 2.0, 1.0  # probe 1: min.y above max.y
    create = rtlib.rt_reflection_probes_create
    # 1. null pointers, with every later fault in the request
    worst = dict(count=0, size=12, levels=0, max_spt=0, pos=bad_pos, box=bad_box)
    assert create(s.h, C.byref(_desc(**worst)), 7, None) == inv and "null" in _err(rtlib)
    assert create(None, C.byref(_desc(**worst)), 7, C.byref(h)) == inv and "null scene" in _err(rtlib) and not h.value
    assert create(s.h, None, 7, C.byref(h)) == inv and "null description" in _err(rtlib)
    assert create(s.h, C.byref(_desc(**dict(worst, pos=None))), 7, C.byref(h)) == inv and "null positions" in _err(rtlib)
    # 2 .. 5. the description's numbers, each with all the later ones
    steps = [("1 .. 4096", {"count": 0}), ("power of two", {"size": 12}), ("levels", {"levels": 0}), ("1 .. 1024", {"max_spt": 0})]
    for first in range(4):
        kw = dict(pos=bad_pos, box=bad_box)
        for _, fault in steps[first:]:
            kw.update(fault)
        h.value = 0x1234
        assert create(s.h, C.byref(_desc(**kw)), 7, C.byref(h)) == inv, kw
        assert steps[first][0] in _err(rtlib), (kw, _err(rtlib))
        assert not h.value  # the output is cleared
    for kw, word in (({"count": 4097}, "1 .. 4096"), ({"count": 0xFFFFFFFF}, "1 .. 4096"), ({"size": 4}, "power of two"), ({"size": 256}, "power of two"),
                     ({"size": 0}, "power of two"), ({"size": 24}, "power of two"), ({"levels": 3}, "levels"), ({"size": 128, "levels": 7}, "levels"),
                     ({"size": 16, "levels": 4}, "levels"), ({"max_spt": 1025}, "1 .. 1024"),
                     # 6. the entry count
                     ({"count": 4096, "size": 128, "levels": 6, "max_spt": 1024}, "2^31"), ({"count": 342, "size": 32, "max_spt": 1024}, "2^31"),
                     ({"count": 22, "size": 128, "max_spt": 1024}, "2^31")):
        assert create(s.h, C.byref(_desc(pos=bad_pos, box=bad_box, **kw)), 7, C.byref(h)) == inv, kw
        assert word in _err(rtlib), (kw, _err(rtlib))
    # 7. the values, with the flag fault behind them
    for kw, word in (({"pos": bad_pos, "box": bad_box}, "position"), ({"box": bad_box}, "min above max")):
        assert create(s.h, C.byref(_desc(**kw)), 7, C.byref(h)) == inv and word in _err(rtlib), (kw, _err(rtlib))
    for v in (nan, inf, -inf):
        p = _POS.copy()
        p[5] = v
        assert create(s.h, C.byref(_desc(pos=p)), 0, C.byref(h)) == inv and "position" in _err(rtlib)
        b = _BOX.copy()
        b[9] = v
        assert create(s.h, C.byref(_desc(box=b)), 0, C.byref(h)) == inv and "box value" in _err(rtlib)
    p = _POS.copy()
    p[6] = nan  # behind the two probes of the request: not read
    assert create(s.h, C.byref(_desc(pos=p)), 0, C.byref(h)) == abi.RT_ERR_NO_DEVICE
    # 8. flags
    assert create(s.h, C.byref(_desc(box=_BOX)), 1, C.byref(h)) == inv and "flag" in _err(rtlib)
    # well formed: the scene has no device
    for kw in ({}, {"box": _BOX}, {"count": 1, "size": 8, "levels": 1, "max_spt": 1}, {"count": 4096, "size": 8, "levels": 2, "max_spt": 1024},
               {"count": 21, "size": 128, "levels": 6, "max_spt": 1024}, {"count": 341, "size": 32, "levels": 4, "max_spt": 1024}):
        h.value = 0x1234
        assert create(s.h, C.byref(_desc(**kw)), 0, C.byref(h)) == abi.RT_ERR_NO_DEVICE, kw
        assert "host-only" in _err(rtlib) and not h.value
    degenerate = _BOX.copy()
    degenerate[:6] = 0.5  # min == max is allowed
    assert create(s.h, C.byref(_desc(box=degenerate)), 0, C.byref(h)) == abi.RT_ERR_NO_DEVICE
    rtlib.rt_reflection_probes_destroy(None)
    s.close()


def test_calls_refuse_null_handles_before_any_device_call(rtlib):
    inv = abi.RT_ERR_INVALID
    buf = np.zeros(64, f32)
    words = np.zeros(16, np.uint32)
    p = abi.rt_reflection_bake_params(4, 5, 0, 1, 0.0)
    st = abi.rt_reflection_stats()
    L = rtlib
    calls = [lambda: L.rt_reflection_probes_entries(None, C.byref(p), abi.fptr(buf), abi.fptr(buf), abi.u32ptr(words)),
             lambda: L.rt_reflection_probes_entries_device(None, C.byref(p), None, None, None, None),
             lambda: L.rt_reflection_probes_bake(None, C.byref(p), abi.fptr(buf), C.byref(st)),
             lambda: L.rt_reflection_probes_bake(None, None, None, None),
             lambda: L.rt_reflection_probes_bake_device(None, C.byref(p), None, None, None),
             lambda: L.rt_reflection_probes_set_level0(None, abi.fptr(buf)),
             lambda: L.rt_reflection_probes_set_level0_device(None, None, None),
             lambda: L.rt_reflection_probes_prefilter(None),
             lambda: L.rt_reflection_probes_prefilter_device(None, None),
             lambda: L.rt_reflection_probes_get_chain(None, abi.fptr(buf)),
             lambda: L.rt_reflection_probes_get_chain_device(None, None, None),
             lambda: L.rt_reflection_probes_sample(None, 4, abi.u32ptr(words), abi.fptr(buf), abi.fptr(buf), abi.fptr(buf), abi.fptr(buf)),
             lambda: L.rt_reflection_probes_sample(None, 0, None, None, None, None, None),
             lambda: L.rt_reflection_probes_sample_device(None, 4, None, None, None, None, None, None)]
    for k, call in enumerate(calls):
        assert call() == inv, k
        assert "null" in _err(rtlib), (k, _err(rtlib))


def test_python_wrapper_refuses_wrong_shapes(rtlib):
    s = Scene(scenes.get_scene("cube"), device=-1)
    pos = np.zeros((2, 3), f32)
    box = np.tile(np.array([[-1, -1, -1, 1, 1, 1]], f32), (2, 1))
    for good in ((pos, 8, 2), ([[0, 0, 0]], 16, 3, 4), (pos.astype(np.float64), 8, 1, 1, box), (pos, 8, 2, 2, box.tolist())):
        with pytest.raises(abi.RtError) as e:
            ReflectionProbes(s, *good)
        assert e.value.status == abi.RT_ERR_NO_DEVICE
    for bad in ((np.zeros(3, f32), 8, 2), (np.zeros((2, 2), f32), 8, 2), (pos, 8, 2, 1, box[:1]), (pos, 8, 2, 1, np.zeros((2, 3), f32)),
                (pos, -8, 2), (pos, 8, -1), (pos, 8, 2, 1 << 32), (np.array([["a", "b", "c"]]), 8, 2)):
        with pytest.raises(ValueError):
            ReflectionProbes(s, *bad)
    for bad in ((np.zeros((0, 3), f32), 8, 2), (pos, 12, 2), (pos, 8, 3), (pos, 8, 2, 0), (np.full((1, 3), np.nan, f32), 8, 2),
                (pos, 8, 2, 1, box[:, ::-1].copy())):
        with pytest.raises(abi.RtError) as e:
            ReflectionProbes(s, *bad)
        assert e.value.status == abi.RT_ERR_INVALID
    import rtamd
    assert rtamd.ReflectionProbes is ReflectionProbes
    s.close()
