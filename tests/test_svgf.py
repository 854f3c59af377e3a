"""CPU tests of variance-guided denoising (rt_temporal_accumulate_moments, rt_denoise_variance, rt_denoise_guided and their _device forms), and the
numpy float32 models that tests/test_gpu_svgf.py pins the device to bit for bit:

    moments_model    rt_temporal_accumulate_moments: temporal_model's colour plus the luminance moments through the same taps
    variance_model   rt_denoise_variance: the moments where the history is long enough, the guided 7 x 7 window elsewhere
    guided_model     rt_denoise_guided: denoise_model with the colour term replaced by |dl| / (sigma_l * sd) and the variance carried along

Every numpy operation below is one IEEE binary32 operation on float32 arrays, in the order include/rt_mi355x.h states (no FMA in numpy)."""
import ctypes as C
import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest

from rtamd import abi

REPO = Path(__file__).resolve().parent.parent
f32 = np.float32
INF = float("inf")


def _load(name):
    spec = importlib.util.spec_from_file_location(f"_svgf_{name}", Path(__file__).with_name(f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_dn = _load("test_denoise")
_tm = _load("test_temporal")
exp_m, coefficient, to_unorm8, denoise_model, gbuffer_model, camera_rays = (_dn.exp_m, _dn.coefficient, _dn.to_unorm8, _dn.denoise_model,
                                                                             _dn.gbuffer_model, _dn.camera_rays)
TAP_H, _dot, _listing = _dn.TAP_H, _dn._dot, _dn._listing
temporal_model, reproject = _tm.temporal_model, _tm.reproject

LUM = (f32(0.2126), f32(0.7152), f32(0.0722))
PRE_K = [f32(0.25), f32(0.5), f32(0.25)]
LUM_EPS = f32(1e-8)


def lum(L):
    return (L[..., 0] * LUM[0] + L[..., 1] * LUM[1]) + L[..., 2] * LUM[2]


# ---- the models ------------------------------------------------------------------------------------------------------------------------
def moments_model(state, frame, gbuf, cam, max_history, sigma_position, cos_normal):
    """One call of rt_temporal_accumulate_moments. `state`: None or what the previous call returned (temporal_model's state plus "moments").
    Returns (out_f32, out_u8, history_len, moments (H, W, 2), new state)."""
    trace = {}
    out, u8, n_new, new_state = temporal_model(state, frame, gbuf, cam, max_history, sigma_position, cos_normal, trace=trace)
    F = np.asarray(frame, f32)
    H, W = F.shape[:2]
    with np.errstate(all="ignore"):
        l = lum(F[..., :3] * F[..., :3])
        M = np.stack([l, l * l], -1).astype(f32)
        if state is not None:
            x0, y0 = np.floor(trace["sx"]).astype(np.int64), np.floor(trace["sy"]).astype(np.int64)
            S = np.zeros((H, W, 2), f32)
            k = 0
            for j in (0, 1):
                for i in (0, 1):
                    tap = trace["taps"][k]
                    k += 1
                    tx, ty = np.clip(x0 + i, 0, W - 1), np.clip(y0 + j, 0, H - 1)
                    Mt = state["moments"][ty, tx]
                    S = np.where(tap["valid"][..., None], S + tap["w"][..., None] * Mt, S)
            Hm = S / trace["wsum"][..., None]
            a = f32(1) / trace["n_next"]
            Mb = Hm + (M - Hm) * a[..., None]
            M = np.where(trace["good"][..., None], Mb, M).astype(f32)
    new_state["moments"] = M
    return out, u8, n_new, M, new_state


def variance_model(frame, gbuf, sigma_normal, sigma_position, sigma_albedo, moments=None, history_len=None, min_history=4):
    """rt_denoise_variance: (H, W) float32."""
    F = np.asarray(frame, f32)
    H, W = F.shape[:2]
    A, N, P = (np.asarray(gbuf[k], f32) for k in ("albedo", "normal", "position"))
    kn, kx, ka = (coefficient(s) for s in (sigma_normal, sigma_position, sigma_albedo))
    hit = np.isfinite(P[..., 3])
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        l = lum(F[..., :3] * F[..., :3])
        s1, s2, ws = (np.zeros((H, W), f32) for _ in range(3))
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                qy, qx = ys + dy, xs + dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                use = inside & (hit[qy, qx] == hit)
                E = np.zeros((H, W), f32)
                if kn != 0:
                    E = E + _dot(N - N[qy, qx]) * kn
                if kx != 0:
                    E = E + _dot(P[..., :3] - P[qy, qx, :3]) * kx
                if ka != 0:
                    E = E + _dot(A - A[qy, qx]) * ka
                w = exp_m(-E)
                lq = l[qy, qx]
                s1 = np.where(use, s1 + w * lq, s1)
                s2 = np.where(use, s2 + w * (lq * lq), s2)
                ws = np.where(use, ws + w, ws)
        m1, m2 = s1 / ws, s2 / ws
        if moments is not None:
            mom = np.asarray(moments, f32)
            temporal = np.asarray(history_len, f32) >= f32(min_history)
            m1, m2 = np.where(temporal, mom[..., 0], m1), np.where(temporal, mom[..., 1], m2)
        return np.fmax(m2 - m1 * m1, f32(0)).astype(f32)


def guided_model(frame, gbuf, variance, iterations, sigma_luminance, sigma_normal, sigma_position, sigma_albedo):
    """(f32 (H, W, 4), u8 (H, W, 4), variance (H, W)) of rt_denoise_guided."""
    frame = np.asarray(frame, f32)
    var = np.asarray(variance, f32).copy()
    H, W = frame.shape[:2]
    if iterations == 0:
        u8 = np.concatenate([to_unorm8(frame[..., :3]), np.full((H, W, 1), 255, np.uint8)], -1)
        return frame.copy(), u8, var
    A, N, P = (np.asarray(gbuf[k], f32) for k in ("albedo", "normal", "position"))
    sl = f32(sigma_luminance)
    kn, kx, ka = (coefficient(s) for s in (sigma_normal, sigma_position, sigma_albedo))
    hit = np.isfinite(P[..., 3])
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        L = frame[..., :3] * frame[..., :3]
        for i in range(iterations):
            s = 1 << i
            kni = f32(np.ldexp(kn, -2 * i))
            l = lum(L)
            if not np.isinf(sl):
                g = np.zeros((H, W), f32)
                for dy in range(-1, 2):
                    for dx in range(-1, 2):
                        g = g + (PRE_K[dy + 1] * PRE_K[dx + 1]) * var[np.clip(ys + dy, 0, H - 1), np.clip(xs + dx, 0, W - 1)]
                kl = f32(1) / (sl * np.sqrt(g) + LUM_EPS)
            S = np.zeros((H, W, 3), f32)
            V = np.zeros((H, W), f32)
            wsum = np.zeros((H, W), f32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = ys + s * dy, xs + s * dx
                    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    use = inside & (hit[qy, qx] == hit)
                    Lq = L[qy, qx]
                    E = np.zeros((H, W), f32)
                    if not np.isinf(sl):
                        E = E + np.abs(l - l[qy, qx]) * kl
                    if kni != 0:
                        E = E + _dot(N - N[qy, qx]) * kni
                    if kx != 0:
                        E = E + _dot(P[..., :3] - P[qy, qx, :3]) * kx
                    if ka != 0:
                        E = E + _dot(A - A[qy, qx]) * ka
                    w = (TAP_H[dy + 2] * TAP_H[dx + 2]) * exp_m(-E)
                    S = np.where(use[..., None], S + w[..., None] * Lq, S)
                    wsum = np.where(use, wsum + w, wsum)
                    V = np.where(use, V + (w * w) * var[qy, qx], V)
            L = S / wsum[..., None]
            var = (V / (wsum * wsum)).astype(f32)
        out = np.concatenate([np.sqrt(L), np.ones((H, W, 1), f32)], -1).astype(f32)
    u8 = np.concatenate([to_unorm8(out[..., :3]), np.full((H, W, 1), 255, np.uint8)], -1)
    return out, u8, var


# ---- declarations and refusals ---------------------------------------------------------------------------------------------------------
NEW = ["rt_temporal_create_ex", "rt_temporal_accumulate_moments", "rt_temporal_accumulate_moments_device", "rt_denoiser_create_ex",
       "rt_denoise_variance", "rt_denoise_variance_device", "rt_denoise_guided", "rt_denoise_guided_device"]


def test_entry_points_are_declared_exported_and_prototyped(rtlib, devlib):
    header = (REPO / "include" / "rt_mi355x.h").read_text()
    for name in NEW:
        assert re.search(rf"\b{name}\(", header), name
        assert name in abi.PROTOTYPES, name
        assert hasattr(rtlib, name) and hasattr(devlib, name), name
    assert "#define RT_TEMPORAL_MOMENTS 1u" in header and abi.RT_TEMPORAL_MOMENTS == 1
    assert "#define RT_DENOISER_VARIANCE 1u" in header and abi.RT_DENOISER_VARIANCE == 1
    assert C.sizeof(abi.rt_denoise_var_params) == 24
    fields = ["iterations", "sigma_luminance", "sigma_normal", "sigma_position", "sigma_albedo", "min_history"]
    assert [f[0] for f in abi.rt_denoise_var_params._fields_] == fields
    body = re.search(r"typedef struct rt_denoise_var_params \{(.*?)\} rt_denoise_var_params;", header, re.S).group(1)
    assert re.findall(r"(?:uint32_t|float) (\w+);", body) == fields
    assert rtlib.rt_abi_version() == 8 and devlib.rt_abi_version() == 8 and "#define RT_ABI_VERSION 8" in header
    from rtamd import renderer
    assert renderer.DENOISE_SIGMA_LUMINANCE == 4.0 and renderer.DENOISE_MIN_HISTORY == 4


def _err(lib):
    e = lib.rt_last_error()
    return e.decode() if isinstance(e, bytes) else str(e)


def test_refusals_come_before_any_device_call(rtlib):
    """No denoiser or accumulator exists here: the calls carry a null handle, and the parameter refusals are told from the handle's by their
    messages (the parameters are judged first, as rt_temporal_accumulate's are)."""
    inv = abi.RT_ERR_INVALID
    buf = np.zeros(16, f32)
    ptr = abi.fptr(buf)
    u8 = abi.u8ptr(np.zeros(16, np.uint8))
    out = C.c_void_p()
    for create in (rtlib.rt_denoiser_create_ex, rtlib.rt_temporal_create_ex):
        assert create(-1, 4, 4, 1, C.byref(out)) == inv and not out.value
        assert create(0, 0, 4, 1, C.byref(out)) == inv
        assert create(0, 4, -1, 1, C.byref(out)) == inv
        assert create(0, 4, 4, 1, None) == inv
        assert create(0, 4, 4, 2, C.byref(out)) == inv and "flag" in _err(rtlib)  # an unknown flag, refused before the device is looked for
        assert create(0, 65536, 32768, 1, C.byref(out)) == inv  # W * H = 2^31
        assert create(0, 1, 2**31 - 1, 1, C.byref(out)) == inv  # the 1-D grid of 64 x 4 tiles would pass 2^32 threads
    good = abi.rt_denoise_var_params(5, 4.0, 0.25, 1.0, 0.1, 4)
    P = C.byref

    def variance(p, host, mom=True, hist=True, o=True):
        if host:
            return rtlib.rt_denoise_variance(None, p, ptr, ptr, ptr, ptr, ptr if mom else None, ptr if hist else None, ptr if o else None)
        return rtlib.rt_denoise_variance_device(None, p, 1, 1, 1, 1, 1 if mom else None, 1 if hist else None, 1 if o else None, None)

    def guided(p, host, f=True, b=True):
        if host:
            return rtlib.rt_denoise_guided(None, p, ptr, ptr, ptr, ptr, ptr, ptr if f else None, u8 if b else None, None)
        return rtlib.rt_denoise_guided_device(None, p, 1, 1, 1, 1, 1, 1 if f else None, 1 if b else None, None, None)

    for host in (True, False):
        for call in (variance, guided):
            assert call(P(good), host) == inv and "null argument" in _err(rtlib)
            assert call(None, host) == inv and "parameters" in _err(rtlib)
            assert call(P(abi.rt_denoise_var_params(11, 4.0, 0.25, 1.0, 0.1, 4)), host) == inv and "iterations" in _err(rtlib)
            for k in range(1, 5):
                for bad in (0.0, 1e-7, -1.0, float("nan"), -INF):
                    v = [5, 4.0, 0.25, 1.0, 0.1, 4]
                    v[k] = bad
                    assert call(P(abi.rt_denoise_var_params(*v)), host) == inv and "sigma" in _err(rtlib), (k, bad)
            for ok in (abi.rt_denoise_var_params(10, INF, INF, INF, INF, 0), abi.rt_denoise_var_params(0, 1e-6, 1e-6, 1e-6, 1e-6, 2**32 - 1)):
                assert call(P(ok), host) == inv and "null argument" in _err(rtlib)  # the limits themselves pass the parameter test
        assert guided(P(good), host, f=False, b=False) == inv and "both null" in _err(rtlib)
        assert variance(P(good), host, o=False) == inv and "null argument" in _err(rtlib)
        assert variance(P(good), host, mom=False) == inv and variance(P(good), host, hist=False) == inv
    # (a denoiser or an accumulator created WITHOUT its flag needs a device to exist: that refusal is tests/test_gpu_svgf.py's)
    # moments without an accumulator
    cam = abi.rt_camera()
    cam.width, cam.height = 2, 2
    tp = abi.rt_temporal_params(8, 1.0, 0.5)
    assert rtlib.rt_temporal_accumulate_moments(None, P(tp), P(cam), ptr, ptr, ptr, ptr, ptr, u8, None, ptr) == inv and "null argument" in _err(rtlib)
    assert rtlib.rt_temporal_accumulate_moments_device(None, P(tp), P(cam), 1, 1, 1, 1, 1, 1, None, 1, None) == inv
    assert rtlib.rt_temporal_accumulate_moments(None, None, P(cam), ptr, ptr, ptr, ptr, ptr, u8, None, ptr) == inv and "parameters" in _err(rtlib)
    bad = abi.rt_temporal_params(0, 1.0, 0.5)
    assert rtlib.rt_temporal_accumulate_moments(None, P(bad), P(cam), ptr, ptr, ptr, ptr, ptr, u8, None, ptr) == inv and "max_history" in _err(rtlib)


# ---- the models' own identities ----------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _synthetic(h, w, seed):
    rng = np.random.default_rng(seed)
    frame = np.ones((h, w, 4), f32)
    frame[..., :3] = rng.random((h, w, 3), dtype=f32) * f32(1.5)
    g = {k: rng.random((h, w, 4), dtype=f32) for k in ("albedo", "normal", "position")}
    g["position"][rng.random((h, w)) < 0.2] = (0, 0, 0, np.inf)
    var = (rng.random((h, w), dtype=f32) * f32(0.3)).astype(f32)
    return frame, g, var


def test_guided_model_without_the_luminance_term_is_the_denoise_model_without_the_colour_term():
    frame, g, var = _synthetic(11, 14, 5)
    for it in (0, 1, 3):
        a, ab, _ = guided_model(frame, g, var, it, INF, 0.3, 0.4, 0.2)
        b, bb = denoise_model(frame, g, it, INF, 0.3, 0.4, 0.2)
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(ab, bb), it


def test_a_constant_image_with_zero_variance_is_a_fixed_point():
    _, g, _ = _synthetic(9, 13, 6)
    c = np.full((9, 13, 4), f32(0.5))
    c[..., 3] = 1
    out, _, var = guided_model(c, g, np.zeros((9, 13), f32), 3, 4.0, 0.5, 0.5, 0.5)
    assert np.allclose(out[..., :3], 0.5, rtol=2e-7) and (var == 0).all()
    # ... and zero variance under a varying image leaves kl = 1 / 1e-8: only equal luminances mix, and the variance stays 0
    frame, g, _ = _synthetic(9, 13, 7)
    out, _, var = guided_model(frame, g, np.zeros((9, 13), f32), 2, 4.0, INF, INF, INF)
    assert (var == 0).all() and np.allclose(out, frame, rtol=1e-6)


def test_variance_of_a_flat_region_shrinks_by_the_sum_of_the_squared_weights():
    """All guides off and a constant image: every weight is h_y * h_x, Wsum = 1, and var' = var * sum((h_y h_x)^2) = var * (sum h^2)^2 away from
    the border (sum h^2 = 35/128)."""
    H = W = 12
    c = np.full((H, W, 4), f32(0.7))
    g = {k: np.zeros((H, W, 4), f32) for k in ("albedo", "normal", "position")}
    var = np.full((H, W), f32(0.25))
    _, _, v1 = guided_model(c, g, var, 1, INF, INF, INF, INF)
    h = np.array([float(x) for x in TAP_H])
    want = 0.25 * float((np.outer(h, h) ** 2).sum())
    assert abs(want - 0.25 * (35 / 128) ** 2) < 1e-15
    assert np.allclose(v1[2:-2, 2:-2], want, rtol=1e-6)
    _, _, v1l = guided_model(c, g, var, 1, 4.0, INF, INF, INF)  # the luminance term is exactly 0 on a constant image
    assert np.array_equal(bits(v1), bits(v1l))


def test_variance_model_takes_the_moments_only_where_the_history_is_long_enough():
    frame, g, _ = _synthetic(10, 12, 8)
    rng = np.random.default_rng(9)
    m1 = rng.random((10, 12), dtype=f32)
    mom = np.stack([m1, m1 * m1 + rng.random((10, 12), dtype=f32) * f32(0.1)], -1).astype(f32)
    n = rng.integers(0, 8, (10, 12)).astype(f32)
    spatial = variance_model(frame, g, 0.3, 0.4, 0.2)
    both = variance_model(frame, g, 0.3, 0.4, 0.2, mom, n, 4)
    with np.errstate(all="ignore"):
        temporal = np.fmax(mom[..., 1] - mom[..., 0] * mom[..., 0], f32(0))
    assert np.array_equal(bits(both), bits(np.where(n >= 4, temporal, spatial)))
    assert (spatial >= 0).all() and (both >= 0).all()
    assert np.array_equal(bits(variance_model(frame, g, 0.3, 0.4, 0.2, mom, n, 0)), bits(temporal))
    assert np.array_equal(bits(variance_model(frame, g, 0.3, 0.4, 0.2, mom, n, 9)), bits(spatial))


def test_non_finite_radiance_does_what_the_header_says():
    """include/rt_mi355x.h, "Non-finite radiance": a 1e20 firefly is L = +inf; the variance estimate gives 0 wherever the window holds it (never NaN);
    the filter turns the colour of every pixel with the firefly among its taps into NaN, as rt_denoise does, and no other; the variance
    only at the firefly itself."""
    H, W = 16, 18
    frame, g, _ = _synthetic(H, W, 10)
    g["position"][..., 3] = 1  # all hits: every window reaches the firefly
    for k in ("normal", "albedo"):
        g[k][:] = 0
    g["position"][..., :3] = 0
    frame[8, 9, :3] = 1e20
    var = variance_model(frame, g, 0.3, 0.4, 0.2)
    assert not np.isnan(var).any()
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    window = (abs(ys - 8) <= 3) & (abs(xs - 9) <= 3)
    assert (var[window] == 0).all() and np.isfinite(var[~window]).all() and (var[~window] > 0).all()
    # moments holding an infinite second moment and a finite first: var = +inf, the one case the header names
    mom = np.zeros((H, W, 2), f32)
    mom[..., 0], mom[..., 1] = 1e19, np.inf
    v = variance_model(frame, g, 0.3, 0.4, 0.2, mom, np.full((H, W), 8, f32), 4)
    assert np.isposinf(v).all()
    mom[..., 0] = np.inf
    assert (variance_model(frame, g, 0.3, 0.4, 0.2, mom, np.full((H, W), 8, f32), 4) == 0).all()
    out, _, ov = guided_model(frame, g, var, 1, 4.0, 0.3, 0.4, 0.2)
    taps = (abs(ys - 8) <= 2) & (abs(xs - 9) <= 2)
    own = (ys == 8) & (xs == 9)
    assert np.isnan(out[taps][:, :3]).all() and np.isfinite(out[~taps]).all()
    assert np.isnan(ov[own]).all() and np.isfinite(ov[~own]).all()  # Wsum = 0 at the firefly itself, and only there
    with np.errstate(all="ignore"):
        ref, _ = denoise_model(frame, g, 1, 1.0, 0.3, 0.4, 0.2)
    assert np.array_equal(np.isnan(ref[..., 0]), taps)
    # a variance of +inf: kl = 0, the luminance term is exactly 0 between finite luminances
    a, _, _ = guided_model(frame * 0 + 0.5, g, np.full((H, W), np.inf, f32), 1, 4.0, 0.3, 0.4, 0.2)
    assert np.isfinite(a).all()


def test_moments_model_is_the_running_mean_of_l_and_l_squared_on_a_static_plane():
    plane_camera, plane_gbuffer, frame_of = _tm.plane_camera, _tm.plane_gbuffer, _tm.frame_of
    cam = plane_camera(0.0)
    g = plane_gbuffer(cam)
    state = None
    ls = []
    for k in range(5):
        fr = frame_of(40 + k)
        out, u8, n, M, state = moments_model(state, fr, g, cam, 32, 1.0, 0.9)
        t_out, t_u8, t_n, _ = temporal_model(None if k == 0 else prev, fr, g, cam, 32, 1.0, 0.9)
        prev = {key: state[key] for key in ("colour", "position", "normal", "cam")}
        assert np.array_equal(bits(out), bits(t_out)) and np.array_equal(u8, t_u8) and np.array_equal(bits(n), bits(t_n))
        ls.append(lum(fr[..., :3].astype(np.float64) ** 2))
        assert (n == k + 1).all()
        assert np.allclose(M[..., 0], np.mean(ls, 0), rtol=1e-5) and np.allclose(M[..., 1], np.mean(np.square(ls), 0), rtol=1e-5)
        if k:  # var' >= a / (1 - a) (l - m1')^2: a frame that lies off the stored mean leaves a positive variance
            m1, m2 = M[..., 0].astype(np.float64), M[..., 1].astype(np.float64)
            apart = np.abs(ls[-1] - m1) > 0.1 * np.maximum(ls[-1], m1)
            assert apart.any() and (m2[apart] - m1[apart] ** 2 > 0).all() and (m2 - m1 * m1 >= -1e-5 * m2).all()


# ---- the contract's quality, on the oracle's frames ------------------------------------------------------------------------------------------
def _linear_rmse(a, ref):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) ** 2 - ref[..., :3].astype(np.float64) ** 2) ** 2)))


@pytest.mark.parametrize("name,kw,bound", [("cornell", {}, 0.6), ("atrium", {"coarse": True}, 1.1)])
def test_guided_defaults_against_denoise_defaults_on_the_oracle_frames(oracle, scene_cache, name, kw, bound):
    """128 x 72, depth 10, 4 spp against 512 spp, megakernel seeds; guides from gbuffer_model; both filters at the defaults of rtamd/renderer.py
    and 5 iterations; the variance is the spatial estimate (a still). RMSE in linear radiance; the ratio guided / rt_denoise must stay under the
    bound."""
    from rtamd import renderer as R
    sd = scene_cache(name, **kw)
    w, h = 128, 72
    osc = oracle.OracleScene(sd)
    cam = oracle.camera(w, h, sd.camera.position, sd.camera.direction, sd.camera.focal_length)
    nt = oracle.hardware_threads()
    raw, _, _ = osc.render(cam, abi.RT_RENDERER_MEGAKERNEL, 10, 4, nthreads=nt)
    ref, _, _ = osc.render(cam, abi.RT_RENDERER_MEGAKERNEL, 10, 512, nthreads=nt)
    org, d = camera_rays(cam)
    g = gbuffer_model(sd, cam, *osc.intersect(org, d, True))
    scale = _scene_scale(sd)
    sp = f32(R.DENOISE_POSITION_FRACTION) * f32(scale)
    plain, _ = denoise_model(raw, g, R.DENOISE_ITERATIONS, R.DENOISE_SIGMA_COLOR, R.DENOISE_SIGMA_NORMAL, sp, R.DENOISE_SIGMA_ALBEDO)
    var = variance_model(raw, g, R.DENOISE_SIGMA_NORMAL, sp, R.DENOISE_SIGMA_ALBEDO)
    guided, _, _ = guided_model(raw, g, var, R.DENOISE_ITERATIONS, R.DENOISE_SIGMA_LUMINANCE, R.DENOISE_SIGMA_NORMAL, sp, R.DENOISE_SIGMA_ALBEDO)
    e_raw, e_plain, e_guided = _linear_rmse(raw, ref), _linear_rmse(plain, ref), _linear_rmse(guided, ref)
    print(f"{name}: raw {e_raw:.4f}, rt_denoise defaults {e_plain:.4f}, guided defaults {e_guided:.4f}, ratio {e_guided / e_plain:.3f} (bound {bound})")
    assert e_guided / e_plain <= bound, (e_raw, e_plain, e_guided)


def _scene_scale(sd):
    """Scene.scale() without a device: the largest extent of the bounds rt_scene_info reports for a host-only scene."""
    from rtamd.renderer import Scene
    s = Scene(sd, device=-1)
    try:
        return s.scale()
    finally:
        s.close()


# ---- listings ----------------------------------------------------------------------------------------------------------------------------
def _kernels(lines):
    """name -> (instruction lines, metadata text) of every kernel of a device listing"""
    out = {}
    meta = "\n".join(lines)
    for i, ln in enumerate(lines):
        m = re.match(r"^(_Z\w+):", ln)
        if not m:
            continue
        end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
        out[m.group(1)] = [x.split(";")[0].strip() for x in lines[i:end]]
    return out, meta


def _metadata(meta, symbol, key):
    at = meta.index(f".name:           {symbol}\n")
    # a kernel's metadata entry: the keys around its .name, up to the next entry's .args
    start = meta.rfind("  - .agpr_count", 0, at)
    stop = meta.find("  - .agpr_count", at)
    entry = meta[start:stop if stop > 0 else len(meta)]
    return int(re.search(rf"\.{key}:\s+(\d+)", entry).group(1))


@pytest.mark.parametrize("unit,names", [("rt_variance.hip", ["k_variance", "k_atrous_guided", "k_guided_copy"]),
                                        ("rt_temporal_moments.hip", ["k_temporal_moments"])])
def test_new_units_have_no_lds_no_scratch_no_atomics_and_pass_the_hazard_scan(tmp_path, unit, names):
    from test_isa_hazards import _check
    lines = _listing(unit, tmp_path)
    assert _check(lines) == {}  # no traversal here: no asm node fetch may appear
    kernels, meta = _kernels(lines)
    for n in names:
        assert any(n in k for k in kernels), (n, list(kernels))
    assert len([k for k in kernels if "k_atrous_guided" in k]) in (0, 4)
    for sym, body in kernels.items():
        assert not any("atomic" in ln for ln in body), sym
        assert not any(ln.startswith(("scratch_", "ds_")) for ln in body), sym
        assert not any(re.match(r"s_\w*(store|atomic|dcache)", ln) for ln in body), sym  # scalar memory is read, never written
        assert _metadata(meta, sym, "private_segment_fixed_size") == 0, sym
        assert _metadata(meta, sym, "group_segment_fixed_size") == 0, sym
    if unit == "rt_temporal_moments.hip":
        body = next(b for k, b in kernels.items() if "k_temporal_moments" in k)
        wide = sum(bool(re.match(r"global_load_dwordx[34]\b", ln)) for ln in body)
        assert wide == 16, wide  # k_temporal's 16, each once; the four moment taps are 8-byte loads beside them
        assert sum(bool(re.match(r"global_load_dwordx2\b", ln)) for ln in body) == 4


def test_k_temporal_keeps_its_16_wide_loads_and_its_symbol(tmp_path):
    lines = _listing("rt_temporal.hip", tmp_path)
    kernels, _ = _kernels(lines)
    assert list(kernels) == ["_ZN12_GLOBAL__N_110k_temporalENS_12TemporalArgsEPK15HIP_vector_typeIfLj4EES4_S4_S4_S4_S4_S4_PS2_S5_S5_S5_PS1_IhLj4EEPf"]
    body = next(iter(kernels.values()))
    assert sum(bool(re.match(r"global_load_dwordx[34]\b", ln)) for ln in body) == 16
    assert not any(re.match(r"global_load_dwordx2\b", ln) for ln in body)  # no moment is fetched here
