"""Lightmap filtering (include/rt_mi355x.h: rt_lightmap_create_ex with RT_LIGHTMAP_FILTER, rt_lightmap_bake_filtered[_device],
rt_lightmap_filter[_device]) without a GPU: the numpy float32 models of the contract's steps 5a and 5b that tests/test_gpu_lightmap_filter.py
pins the device to bit for bit,

    lm_variance_model   step 5a: the variance of a sampled texel's mean luminance from its `repeats` entries
    lm_filter_model     step 5b: the a-trous iterations in texel space over a mask plane, guided by world position and shading normal

what the models themselves must show (derived, not measured), and the library in front of the device: the exported symbols, the struct, the
refusals, the wrappers' shape checks. Every numpy operation in the models is one IEEE binary32 operation on float32 arrays, in the order the
header states (no FMA in numpy)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rtamd import abi, bake, scenes
from rtamd import renderer as R
from rtamd.renderer import Lightmap, Scene
from test_denoise import TAP_H, _dot, coefficient, exp_m
from test_svgf import LUM_EPS, PRE_K, guided_model, lum

REPO = Path(__file__).resolve().parent.parent
f32 = np.float32
INF = float("inf")
SYMBOLS = ["rt_lightmap_create_ex", "rt_lightmap_bake_filtered", "rt_lightmap_bake_filtered_device", "rt_lightmap_filter",
           "rt_lightmap_filter_device"]


# ---- the models both files share ---------------------------------------------------------------------------------------------------------
def lm_variance_model(radiance, repeats, sampled):
    """Step 5a: (n,) float32 from the gather's radiance over the n * repeats entries and the (n,) mask of sampled texels"""
    n = len(sampled)
    l = lum(np.asarray(radiance, f32).reshape(n, repeats, 3))
    var = np.zeros(n, f32)
    if repeats > 1:
        with np.errstate(all="ignore"):
            t = np.zeros(n, f32)
            for k in range(repeats):
                t = t + l[:, k]
            m = t / f32(repeats)
            s = np.zeros(n, f32)
            for k in range(repeats):
                d = l[:, k] - m
                s = s + d * d
            var = s / (f32(repeats) * f32(repeats - 1))
    out = np.where(sampled, var, f32(0)).astype(f32)
    assert out.dtype == f32
    return out


def _taps(H, W, dy, dx, mask):
    """the tap (x + dx, y + dy) of every texel: (qy, qx) clipped into the atlas, and use: inside the atlas and in the mask"""
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    qy, qx = ys + dy, xs + dx
    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
    qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
    return qy, qx, inside & mask[qy, qx]


def lm_filter_model(rgb, var, mask, pos, nrm, iterations, sigma_luminance, sigma_normal, sigma_position):
    """Step 5b on (H, W, 3) radiance, (H, W) variance (None: zeros), the (H, W) mask M and the (H, W, 3) guides
    -> (rgba (H, W, 4): alpha 1 on M, zeros elsewhere; variance (H, W): 0 outside M)"""
    mask = np.asarray(mask, bool)
    H, W = mask.shape
    L = np.where(mask[..., None], np.asarray(rgb, f32), f32(0)).astype(f32)
    v = np.where(mask, np.zeros((H, W), f32) if var is None else np.asarray(var, f32), f32(0)).astype(f32)
    P, N = np.asarray(pos, f32), np.asarray(nrm, f32)
    sl = f32(sigma_luminance)
    kn, kx = coefficient(sigma_normal), coefficient(sigma_position)
    with np.errstate(all="ignore"):
        for i in range(iterations):
            s = 1 << i
            kni = f32(np.ldexp(kn, -2 * i))
            l = lum(L)
            if not np.isinf(sl):
                G, K = np.zeros((H, W), f32), np.zeros((H, W), f32)
                for dy in range(-1, 2):
                    for dx in range(-1, 2):
                        qy, qx, use = _taps(H, W, dy, dx, mask)
                        k = PRE_K[dy + 1] * PRE_K[dx + 1]
                        G = np.where(use, G + k * v[qy, qx], G)
                        K = np.where(use, K + k, K)
                kl = f32(1) / (sl * np.sqrt(G / K) + LUM_EPS)
            S, V, wsum = np.zeros((H, W, 3), f32), np.zeros((H, W), f32), np.zeros((H, W), f32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx, use = _taps(H, W, s * dy, s * dx, mask)
                    Lq = L[qy, qx]
                    E = np.zeros((H, W), f32)
                    if not np.isinf(sl):
                        E = E + np.abs(l - l[qy, qx]) * kl
                    if kni != 0:
                        E = E + _dot(N - N[qy, qx]) * kni
                    if kx != 0:
                        E = E + _dot(P - P[qy, qx]) * kx
                    w = (TAP_H[dy + 2] * TAP_H[dx + 2]) * exp_m(-E)
                    S = np.where(use[..., None], S + w[..., None] * Lq, S)
                    wsum = np.where(use, wsum + w, wsum)
                    V = np.where(use, V + (w * w) * v[qy, qx], V)
            L = np.where(mask[..., None], S / wsum[..., None], f32(0)).astype(f32)
            v = np.where(mask, V / (wsum * wsum), f32(0)).astype(f32)
    rgba = np.concatenate([L, mask[..., None].astype(f32)], -1)
    assert rgba.dtype == f32 and v.dtype == f32
    return rgba, v


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- the models alone --------------------------------------------------------------------------------------------------------------------
def test_variance_model_is_zero_for_one_repeat_and_the_sample_variance_of_the_mean_otherwise():
    g = np.random.default_rng(1)
    n = 500
    on = np.ones(n, bool)
    assert (lm_variance_model(g.random((n, 3), dtype=f32), 1, on) == 0).all()
    for r in range(2, 9):
        rad = g.random((n, r, 3), dtype=f32) * f32(2)
        got = lm_variance_model(rad.reshape(-1, 3), r, on)
        l64 = lum(rad).astype(np.float64)
        want = l64.var(axis=1, ddof=1) / r
        # fp32 rounding: m carries r roundings of l <= 2, every difference one more, and the differences are ~ 0.3: 2r + 3 roundings of
        # 2^-24 on terms that do not cancel, so 1e-5 relative; 1e-12 absolute for entries that happen to lie within 1e-3 of each other
        assert np.allclose(got, want, rtol=1e-5, atol=1e-12), r
        off = g.random(n) < 0.3
        np.testing.assert_array_equal(lm_variance_model(rad.reshape(-1, 3), r, ~off), np.where(off, f32(0), got))


def test_equal_entries_give_zero_variance():
    """R equal entries of luminance l. R = 2: l + l and its half are exact, so m = l, both differences are 0 and var is exactly 0. From
    R = 3 on the sum in order passes through 3l, which needs two more bits than l and may round, so m may miss l: each partial sum carries
    at most 2^-24 relative, |m - l| <= R * 2^-24 * l, the difference l - m is exact (Sterbenz), and var = s / (R (R - 1)) <=
    (R * 2^-24 * l)^2: zero to fp32 rounding (14 orders below l^2), not bit for bit. Black entries give exactly 0 for every R."""
    g = np.random.default_rng(2)
    n = 2000
    on = np.ones(n, bool)
    for r in range(2, 9):
        one = g.random((n, 1, 3), dtype=f32) * f32(3)
        var = lm_variance_model(np.repeat(one, r, 1).reshape(-1, 3), r, on)
        l = lum(one[:, 0]).astype(np.float64)
        if r == 2:
            assert (var == 0).all(), r
        else:
            assert (var <= 1.01 * (r * 2.0 ** -24 * l) ** 2).all(), r
    black = np.zeros((n * 3, 3), f32)
    assert (lm_variance_model(black, 3, on) == 0).all()


def _guides(H, W, seed):
    g = np.random.default_rng(seed)
    return g.random((H, W, 3), dtype=f32), g.random((H, W, 3), dtype=f32)


def test_a_constant_plane_is_a_fixed_point_whatever_its_variance():
    """S = sum(w * c) and Wsum = sum(w): with c a power of two every product and every partial sum of S is the matching one of Wsum scaled
    exactly, so S / Wsum = c bit for bit, whatever the weights. Another constant returns to within the 26 roundings of the two sums."""
    H, W = 9, 13
    g = np.random.default_rng(3)
    P, N = _guides(H, W, 4)
    mask = g.random((H, W)) < 0.8
    var = (g.random((H, W), dtype=f32) * f32(0.3)).astype(f32)
    c = np.broadcast_to(np.array([0.5, 2.0, 0.125], f32), (H, W, 3))
    for sig in ((4.0, 0.5, 0.5), (INF, 0.5, INF), (4.0, INF, INF)):
        out, v = lm_filter_model(c, var, mask, P, N, 3, *sig)
        np.testing.assert_array_equal(bits(out[mask][:, :3]), bits(c[mask]))
        assert (out[mask][:, 3] == 1).all() and (out[~mask] == 0).all() and (v[~mask] == 0).all() and (v[mask] >= 0).all()
    c = np.broadcast_to(np.array([0.3, 0.7, 1.1], f32), (H, W, 3))
    out, _ = lm_filter_model(c, var, mask, P, N, 3, 4.0, 0.5, 0.5)
    assert np.allclose(out[mask][:, :3], c[mask], rtol=3 * 26 * 2.0 ** -24, atol=0)


def test_variance_of_a_flat_region_shrinks_by_the_sum_of_the_squared_weights():
    H = W = 12
    c = np.full((H, W, 3), f32(0.7))
    P, N = _guides(H, W, 5)
    var = np.full((H, W), f32(0.25))
    _, v1 = lm_filter_model(c, var, np.ones((H, W), bool), P, N, 1, INF, INF, INF)
    h = np.array([float(x) for x in TAP_H])
    w = np.outer(h, h)
    want = 0.25 * float((w ** 2).sum()) / float(w.sum()) ** 2
    assert abs(want - 0.25 * (35 / 128) ** 2) < 1e-15
    assert np.allclose(v1[2:-2, 2:-2], want, rtol=1e-6)  # all 25 taps inside the atlas
    corner = w[2:, 2:]
    assert np.isclose(v1[0, 0], 0.25 * float((corner ** 2).sum()) / float(corner.sum()) ** 2, rtol=1e-6)  # 9 taps, renormalised


def test_no_bleed_between_neighbours_in_the_atlas_that_are_far_apart_in_the_world():
    """Two rectangles side by side in the atlas, at least 10 world units apart, sigma_position = 0.1: every cross tap has
    E >= dot * kx >= 100 * 100 = 10^4 > 87, where exp_m is exactly 0, so w = 0 and the tap adds +0 to S, Wsum and V. Changing every value
    and variance of one rectangle leaves the other's output bit-identical: with the luminance term off at every texel, with it on at every
    texel whose 3 x 3 variance prefilter stays on its side (the prefilter has no guides: the header says so)."""
    H, W = 12, 20
    g = np.random.default_rng(6)
    P, N = _guides(H, W, 7)
    P[:, 10:, 0] += f32(11.0)  # the right rectangle: x in [11, 12), the left in [0, 1)
    mask = np.ones((H, W), bool)
    rgb = g.random((H, W, 3), dtype=f32)
    var = (g.random((H, W), dtype=f32) * f32(0.2)).astype(f32)
    a, va = lm_filter_model(rgb, var, mask, P, N, 4, 4.0, 0.5, 0.1)
    rgb2, var2 = rgb.copy(), var.copy()
    rgb2[:, 10:] = g.random((H, 10, 3), dtype=f32) * f32(50)
    var2[:, 10:] = f32(7.0)
    b, vb = lm_filter_model(rgb2, var2, mask, P, N, 4, INF, 0.5, 0.1)
    a_inf, va_inf = lm_filter_model(rgb, var, mask, P, N, 4, INF, 0.5, 0.1)
    np.testing.assert_array_equal(bits(a_inf[:, :10]), bits(b[:, :10]))
    np.testing.assert_array_equal(bits(va_inf[:, :10]), bits(vb[:, :10]))
    assert not np.array_equal(a_inf[:, 10:], b[:, 10:])
    # with the luminance term the 3 x 3 variance prefilter is the one thing that crosses (it has no guides): one column beside the seam
    # sees the other side's variance, and what it changes travels two steps per iteration: the columns beyond that are bit-identical
    c, vc = lm_filter_model(rgb2, var2, mask, P, N, 1, 4.0, 0.5, 0.1)
    a1, va1 = lm_filter_model(rgb, var, mask, P, N, 1, 4.0, 0.5, 0.1)
    np.testing.assert_array_equal(bits(a1[:, :9]), bits(c[:, :9]))
    np.testing.assert_array_equal(bits(va1[:, :9]), bits(vc[:, :9]))
    assert np.isfinite(a).all() and np.isfinite(va).all()


def test_texels_outside_the_mask_come_out_as_zeros_and_are_never_read():
    H, W = 11, 14
    g = np.random.default_rng(8)
    P, N = _guides(H, W, 9)
    mask = g.random((H, W)) < 0.6
    rgb = g.random((H, W, 3), dtype=f32)
    var = (g.random((H, W), dtype=f32) * f32(0.2)).astype(f32)
    for it in (0, 1, 3):
        a, va = lm_filter_model(rgb, var, mask, P, N, it, 4.0, 0.5, 0.5)
        assert (a[~mask] == 0).all() and (va[~mask] == 0).all() and (a[mask][:, 3] == 1).all()
        rgb2, var2, P2, N2 = rgb.copy(), var.copy(), P.copy(), N.copy()
        rgb2[~mask], var2[~mask], P2[~mask], N2[~mask] = np.nan, np.nan, np.nan, np.nan
        b, vb = lm_filter_model(rgb2, var2, mask, P2, N2, it, 4.0, 0.5, 0.5)
        np.testing.assert_array_equal(bits(a), bits(b))
        np.testing.assert_array_equal(bits(va), bits(vb))
    a0, v0 = lm_filter_model(rgb, None, mask, P, N, 0, INF, INF, INF)
    np.testing.assert_array_equal(a0[mask][:, :3], rgb[mask])
    assert (v0 == 0).all()


def test_on_a_full_mask_the_interior_is_the_guided_models_arithmetic():
    """guided_model (tests/test_svgf.py) squares its frame and returns the square root; its albedo term is off at sigma_albedo = inf and its
    mask is full where every position's .w is finite. The two differ in the variance prefilter alone: clamped addresses there, taps outside
    the atlas left out and the sum renormalised here. They coincide where the 3 x 3 window lies inside the atlas (K = 1 exactly, g / 1 = g):
    texels at least 1 from the border after one iteration. The second iteration's taps reach 4 texels out and must land on such texels,
    and its prefilter one more: texels at least 5 from the border after two."""
    H, W = 17, 19
    g = np.random.default_rng(10)
    frame = np.ones((H, W, 4), f32)
    frame[..., :3] = (g.integers(1, 96, size=(H, W, 3)) / 64).astype(f32)  # 7 bits: the square is exact, and is this model's input
    rgb = frame[..., :3] * frame[..., :3]
    gb = {k: g.random((H, W, 4), dtype=f32) for k in ("albedo", "normal", "position")}
    var = (g.random((H, W), dtype=f32) * f32(0.3)).astype(f32)
    full = np.ones((H, W), bool)
    for it, m in ((1, 1), (2, 5)):
        want, _, want_v = guided_model(frame, gb, var, it, 4.0, 0.3, 0.4, INF)
        got, got_v = lm_filter_model(rgb, var, full, gb["position"][..., :3], gb["normal"][..., :3], it, 4.0, 0.3, 0.4)
        inner = (slice(m, H - m), slice(m, W - m))
        with np.errstate(all="ignore"):
            np.testing.assert_array_equal(bits(np.sqrt(got[..., :3])[inner]), bits(want[..., :3][inner]))
        np.testing.assert_array_equal(bits(got_v[inner]), bits(want_v[inner]))
        assert not np.array_equal(got_v, want_v)  # the border differs: the renormalised prefilter
    # without the luminance term there is no prefilter: the whole plane agrees
    want, _, want_v = guided_model(frame, gb, var, 3, INF, 0.3, 0.4, INF)
    got, got_v = lm_filter_model(rgb, var, full, gb["position"][..., :3], gb["normal"][..., :3], 3, INF, 0.3, 0.4)
    np.testing.assert_array_equal(bits(np.sqrt(got[..., :3])), bits(want[..., :3]))
    np.testing.assert_array_equal(bits(got_v), bits(want_v))


# ---- the library in front of the device --------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_prototyped(rtlib, devlib, tmp_path):
    """The test that fails without the feature: the five new functions, the flag and the struct."""
    header = (REPO / "include" / "rt_mi355x.h").read_text()
    assert "#define RT_LIGHTMAP_FILTER 1u" in header and abi.RT_LIGHTMAP_FILTER == 1
    for name in SYMBOLS:
        assert re.search(rf"^(int|void) +{name}\(", header, re.M), name
        assert name in abi.PROTOTYPES
        for lib in (rtlib, devlib):
            assert hasattr(lib, name), name
    assert rtlib.rt_abi_version() == 8 and "#define RT_ABI_VERSION 8" in header
    ff = [f[0] for f in abi.rt_lightmap_filter_params._fields_]
    assert ff == ["iterations", "sigma_luminance", "sigma_normal", "sigma_position"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_mi355x.h"\nint main(void){' +
                   'printf("%zu %zu %zu\\n", sizeof(rt_lightmap_filter_params), sizeof(rt_lightmap_params), sizeof(rt_lightmap_stats));' +
                   "".join(f'printf("%zu\\n", offsetof(rt_lightmap_filter_params, {f}));' for f in ff) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", str(REPO / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [16, 24, 24] + [getattr(abi.rt_lightmap_filter_params, f).offset for f in ff] == [16, 24, 24, 0, 4, 8, 12]
    assert C.sizeof(abi.rt_lightmap_filter_params) == 16


def _err(lib):
    return lib.rt_last_error().decode()


def test_create_ex_refuses_unknown_flags_and_is_create_for_flags_zero(rtlib):
    sd = scenes.get_scene("cube")
    s = Scene(sd, device=-1)
    uv = bake.triangle_grid_uvs(sd.n_triangles, 64, 64).reshape(-1)
    h = C.c_void_p(0x1234)
    for flags in (2, 3, 0x80000000, 0xFFFFFFFF):
        h.value = 0x1234
        assert rtlib.rt_lightmap_create_ex(s.h, 64, 64, 1, abi.fptr(uv), flags, C.byref(h)) == abi.RT_ERR_INVALID
        assert "flag" in _err(rtlib) and not h.value
    for flags in (0, abi.RT_LIGHTMAP_FILTER):  # well-formed: only the device is missing
        assert rtlib.rt_lightmap_create_ex(s.h, 64, 64, 1, abi.fptr(uv), flags, C.byref(h)) == abi.RT_ERR_NO_DEVICE
        assert "host-only" in _err(rtlib) and not h.value
        assert rtlib.rt_lightmap_create_ex(s.h, 0, 64, 1, abi.fptr(uv), flags, C.byref(h)) == abi.RT_ERR_INVALID and "1 .. 8192" in _err(rtlib)
        assert rtlib.rt_lightmap_create_ex(s.h, 64, 64, 0, abi.fptr(uv), flags, C.byref(h)) == abi.RT_ERR_INVALID and "max_repeats" in _err(rtlib)
    assert rtlib.rt_lightmap_create_ex(None, 64, 64, 1, abi.fptr(uv), 1, C.byref(h)) == abi.RT_ERR_INVALID and "null scene" in _err(rtlib)
    assert rtlib.rt_lightmap_create_ex(s.h, 64, 64, 1, abi.fptr(uv), 1, None) == abi.RT_ERR_INVALID and "null" in _err(rtlib)
    s.close()


def _fp(iterations=5, sl=4.0, sn=0.25, sx=0.5):
    return abi.rt_lightmap_filter_params(iterations, sl, sn, sx)


BAD_FILTERS = [({"iterations": 11}, "iterations"), ({"iterations": 0xFFFFFFFF}, "iterations"), ({"sl": float("nan")}, "sigma"),
               ({"sn": float("nan")}, "sigma"), ({"sx": float("nan")}, "sigma"), ({"sl": 0.0}, "sigma"), ({"sn": 9e-7}, "sigma"),
               ({"sx": -1.0}, "sigma"), ({"sx": -INF}, "sigma"), ({"iterations": 0, "sl": 0.0}, "sigma")]
GOOD_FILTERS = [{}, {"iterations": 0}, {"iterations": 10}, {"sl": INF, "sn": INF, "sx": INF}, {"sl": 1e-6, "sn": 1e-6, "sx": 1e-6}]


def test_the_filtered_bake_refuses_bad_parameters_before_the_handle(rtlib):
    """No lightmap exists without a device, so the handle is NULL throughout: the parameters are judged in front of it, each cause named."""
    inv = abi.RT_ERR_INVALID
    buf = np.zeros(16, f32)
    st = abi.rt_lightmap_stats()

    def params(samples=4, max_depth=5, rr_start=0, repeats=2, seed=1, dilate=0):
        return abi.rt_lightmap_params(samples, max_depth, rr_start, repeats, seed, dilate)

    for call in (lambda p, f: rtlib.rt_lightmap_bake_filtered(None, p, f, abi.fptr(buf), abi.fptr(buf), C.byref(st)),
                 lambda p, f: rtlib.rt_lightmap_bake_filtered_device(None, p, f, None, None, None, None)):
        assert call(None, C.byref(_fp())) == inv and "null parameters" in _err(rtlib)
        for kw, word in (({"samples": 0}, "samples"), ({"max_depth": 0}, "max_depth"), ({"repeats": 0}, "repeats"), ({"dilate": 17}, "dilate")):
            assert call(C.byref(params(**kw)), C.byref(_fp())) == inv and word in _err(rtlib), kw
        for kw, word in BAD_FILTERS:
            assert call(C.byref(params()), C.byref(_fp(**kw))) == inv, kw
            assert word in _err(rtlib), (kw, _err(rtlib))
        # one repeat has no noise estimate: refused with the luminance term on and an iteration to run, else not
        assert call(C.byref(params(repeats=1)), C.byref(_fp())) == inv and "repeats >= 2" in _err(rtlib)
        assert call(C.byref(params(repeats=1)), C.byref(_fp(sl=1e-6, iterations=1))) == inv and "repeats >= 2" in _err(rtlib)
        for p, f in ((params(repeats=1), _fp(sl=INF)), (params(repeats=1), _fp(iterations=0)), (params(repeats=1), None)):
            assert call(C.byref(p), C.byref(f) if f is not None else None) == inv and "null argument" in _err(rtlib)
        for kw in GOOD_FILTERS:  # well-formed parameters: the NULL handle is what is left to refuse
            assert call(C.byref(params()), C.byref(_fp(**kw))) == inv and "null argument" in _err(rtlib), kw
        assert call(C.byref(params()), None) == inv and "null argument" in _err(rtlib)  # no filter parameters: the identity, allowed


def test_the_filter_refuses_bad_parameters_before_the_handle(rtlib):
    inv = abi.RT_ERR_INVALID
    buf = np.zeros(16, f32)
    for call in (lambda f, var=True: rtlib.rt_lightmap_filter(None, f, abi.fptr(buf), abi.fptr(buf) if var else None, abi.fptr(buf), None),
                 lambda f, var=True: rtlib.rt_lightmap_filter_device(None, f, None, C.c_void_p(buf.ctypes.data) if var else None, None, None,
                                                                     None)):
        assert call(None) == inv and "null parameters" in _err(rtlib)
        for kw, word in BAD_FILTERS:
            assert call(C.byref(_fp(**kw))) == inv, kw
            assert word in _err(rtlib), (kw, _err(rtlib))
        for kw in ({}, {"iterations": 0}, {"sl": 1e-6}):
            assert call(C.byref(_fp(**kw)), var=False) == inv and "variance may be null only" in _err(rtlib), kw
        assert call(C.byref(_fp(sl=INF)), var=False) == inv and "null argument" in _err(rtlib)
        for kw in GOOD_FILTERS:
            assert call(C.byref(_fp(**kw))) == inv and "null argument" in _err(rtlib), kw


def test_python_wrappers_refuse_wrong_shapes_and_dtypes(rtlib):
    sd = scenes.get_scene("cube")
    s = Scene(sd, device=-1)
    uv = bake.triangle_grid_uvs(sd.n_triangles, 64, 64)
    with pytest.raises(abi.RtError) as e:
        Lightmap(s, uv, 64, 64, filter=True)
    assert e.value.status == abi.RT_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        Lightmap(s, uv[:-1], 64, 64, filter=True)
    # no lightmap exists without a device: the wrapper's own checks run in front of the library on an object without a handle
    lm = Lightmap.__new__(Lightmap)
    lm._lib, lm.scene, lm.width, lm.height, lm.max_repeats, lm.h = rtlib, s, 7, 5, 2, C.c_void_p()
    rgba, var = np.zeros((5, 7, 4), f32), np.zeros((5, 7), f32)
    bad = [(rgba[:4], var), (rgba.reshape(7, 5, 4), var), (rgba[..., :3], var), (rgba.astype(np.float64), var), (rgba.reshape(-1), var),
           (rgba, var[:4]), (rgba, var.T), (rgba, var.astype(np.float64)), (rgba, var[..., None]), (np.zeros((5, 14, 4), f32)[:, ::2], var),
           (rgba.tolist(), var)]
    for a, v in bad:
        with pytest.raises(ValueError):
            lm.filter(a, v)
    for out in (np.zeros((5, 7, 3), f32), np.zeros((5, 7, 4), np.float64)):
        with pytest.raises(ValueError):
            lm.filter(rgba, var, out_rgba=out)
    with pytest.raises(abi.RtError) as e:  # well-formed: the library refuses the missing handle
        lm.filter(rgba, var)
    assert e.value.status == abi.RT_ERR_INVALID and "null argument" in str(e.value)
    with pytest.raises(abi.RtError) as e:
        lm.filter(rgba, None)
    assert "variance may be null only" in str(e.value)
    with pytest.raises(abi.RtError) as e:
        lm.bake_filtered(4, 5, 1, repeats=1)
    assert "repeats >= 2" in str(e.value)
    with pytest.raises(abi.RtError) as e:
        lm.bake_filtered(4, 5, 1, iterations=11)
    assert "iterations" in str(e.value)
    lm.h = C.c_void_p()
    s.close()
    # the defaults are the image filter's, sigma_position a fraction of the scene's scale in fp32
    p = R.lightmap_filter_params(scene_scale=f32(12.5))
    assert (p.iterations, p.sigma_luminance, p.sigma_normal) == (R.LIGHTMAP_FILTER_ITERATIONS, R.LIGHTMAP_SIGMA_LUMINANCE, R.LIGHTMAP_SIGMA_NORMAL)
    assert f32(p.sigma_position) == f32(R.LIGHTMAP_POSITION_FRACTION) * f32(12.5)
    assert R.lightmap_filter_params(sigma_position=0.3).sigma_position == f32(0.3)
    with pytest.raises(ValueError):
        R.lightmap_filter_params()
