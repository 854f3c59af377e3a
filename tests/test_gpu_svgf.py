"""GPU tests of variance-guided denoising: rt_temporal_accumulate_moments, rt_denoise_variance and rt_denoise_guided (host and _device forms),
each pinned bit for bit to the numpy float32 models of tests/test_svgf.py, the refusals that need a live handle, the CLI's --guided, and one
reported quality sequence."""
import ctypes as C
import importlib.util
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rtamd import abi
from rtamd.glb_export import export_glb
from rtamd.renderer import (DENOISE_MIN_HISTORY, DENOISE_SIGMA_LUMINANCE, Camera, Denoiser, MegakernelRenderer, Scene, TemporalAccumulator,
                            WavefrontRenderer, denoise_var_params, temporal_params)

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
EXE = REPO / "sycl-ray-tracer_amd" / "host" / "build" / "raytracer"
f32 = np.float32
INF = float("inf")


def _load(name):
    spec = importlib.util.spec_from_file_location(f"_gpu_svgf_{name}", Path(__file__).with_name(f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_m = _load("test_svgf")
moments_model, variance_model, guided_model, _synthetic = _m.moments_model, _m.variance_model, _m.guided_model, _m._synthetic
spin_about_centre = _load("test_scene_update").spin_about_centre


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_bits_or_nan(a, b):
    """bit for bit where the model is a number, NaN where it is NaN (a NaN's payload is not part of the contract)"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def _status(fn):
    with pytest.raises(abi.RtError) as e:
        fn()
    return e.value.status


def linear_rmse(a, ref):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) ** 2 - ref[..., :3].astype(np.float64) ** 2) ** 2)))


# ---- temporal moments ----------------------------------------------------------------------------------------------------------------------
def render_sequence(sd0, w, h, n_frames, spin=3.0, spp=2, depth=6):
    """[(frame, motion G-buffer, camera)] of n_frames frames, salts 1 .. n, the instances turned by `spin` degrees more per frame; also the
    scene's scale."""
    s = Scene(sd0, device=0, updatable=True, keep_previous=True)
    r = MegakernelRenderer(s, (w, h), depth, spp)
    cam = Camera.for_scene(sd0, (w, h))
    out = []
    for f in range(n_frames):
        if f:
            s.update(instances=spin_about_centre(sd0, spin * f))
        r.set_frame_seed(f + 1)
        out.append((r.render_frame(cam, want_u8=False).rgba_f32, s.gbuffer_motion(cam), cam))
    scale = s.scale()
    r.close(), s.close()
    return out, scale


@pytest.mark.parametrize("name,w,h", [("atrium", 64, 36), ("cornell", 48, 32)])
def test_moments_equal_the_model_over_a_sequence_and_the_colour_is_the_plain_accumulators(rtlib, scene_cache, name, w, h):
    seq, scale = render_sequence(scene_cache(name), w, h, 8)
    p = temporal_params(scene_scale=scale)
    kw = dict(max_history=p.max_history, sigma_position=p.sigma_position, cos_normal=p.cos_normal)
    acc, plain, mixed = TemporalAccumulator(0, w, h, moments=True), TemporalAccumulator(0, w, h), TemporalAccumulator(0, w, h, moments=True)
    state = None
    for f, (frame, g, cam) in enumerate(seq):
        r = acc.accumulate(frame, g, cam, **kw)
        mo, mb, mn, mm, state = moments_model(state, frame, g, cam.c, p.max_history, p.sigma_position, p.cos_normal)
        assert same_bits(r["moments"], mm), (f, np.argwhere(r["moments"].view(np.uint32) != mm.view(np.uint32))[:4])
        assert same_bits(r["f32"], mo) and same_bits(r["u8"], mb) and same_bits(r["history_len"], mn), f
        po, pb, pn = plain.accumulate(frame, g, cam, **kw)
        assert same_bits(r["f32"], po) and same_bits(r["u8"], pb) and same_bits(r["history_len"], pn), f
        # a plain call on an accumulator that has moments keeps them: every other frame goes through rt_temporal_accumulate
        if f % 2:
            xo, xb, xn = mixed.accumulate(frame, g, cam, moments=False, **kw)
            assert same_bits(xo, po) and same_bits(xb, pb) and same_bits(xn, pn), f
        else:
            assert same_bits(mixed.accumulate(frame, g, cam, **kw)["moments"], mm), f
    assert r["history_len"].max() == 8
    # The moments do carry a variance. With history, M' = Hm + (M - Hm) a gives var' = (1 - a) var_h + a (1 - a) (l - Hm1)^2 and
    # l - m1' = (1 - a)(l - Hm1), so var' >= a / (1 - a) (l - m1')^2 >= (l - m1')^2 / 7 for n <= 8: where the last frame's luminance lies more
    # than 10 % off the stored mean, the variance exceeds 1e-3 of the larger one's square, far above the rounding of m2 and m1 * m1 (about
    # 8 * 2^-24 relative). How many pixels that is depends on the scene (most of a 2-spp Cornell box is black in every frame): some must exist.
    m1, m2 = r["moments"][..., 0].astype(np.float64), r["moments"][..., 1].astype(np.float64)
    l = _m.lum(np.square(seq[-1][0][..., :3].astype(np.float64)))
    apart = (r["history_len"] >= 2) & (np.abs(l - m1) > 0.1 * np.maximum(l, m1))
    assert apart.any() and (m2[apart] - m1[apart] ** 2 > 0).all()
    assert (m2 - m1 * m1 >= -1e-5 * m2).all()  # Jensen, to rounding: both means use the same weights
    for a in (acc, plain, mixed):
        a.close()


def test_moments_device_variant_in_place_reset_and_the_missing_flag(rtlib, scene_cache):
    import torch
    w, h = 65, 35
    seq, scale = render_sequence(scene_cache("atrium"), w, h, 3)
    p = temporal_params(scene_scale=scale)
    kw = dict(max_history=p.max_history, sigma_position=p.sigma_position, cos_normal=p.cos_normal)
    host, dev = TemporalAccumulator(0, w, h, moments=True), TemporalAccumulator(0, w, h, moments=True)
    st = torch.cuda.Stream(device=0)
    for f, (frame, g, cam) in enumerate(seq):
        r = host.accumulate(frame, g, cam, **kw)
        df = torch.from_numpy(frame).to("cuda:0")
        planes = [torch.from_numpy(np.ascontiguousarray(g[k])).to("cuda:0") for k in ("normal", "position", "prev_position")]
        dm = torch.zeros((h, w, 2), dtype=torch.float32, device="cuda:0")
        dn = torch.zeros((h, w), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        dev.accumulate_moments_device(cam, df.data_ptr(), *(x.data_ptr() for x in planes), dm.data_ptr(), d_out_f32=df.data_ptr(),
                                      d_history_len=dn.data_ptr(), stream=st.cuda_stream, **kw)  # in place on the device
        st.synchronize()
        assert same_bits(df.cpu().numpy(), r["f32"]) and same_bits(dm.cpu().numpy(), r["moments"]) and same_bits(dn.cpu().numpy(), r["history_len"]), f
    host.reset()
    frame, g, cam = seq[2]
    r = host.accumulate(frame, g, cam, **kw)
    _, _, _, mm, _ = moments_model(None, frame, g, cam.c, p.max_history, p.sigma_position, p.cos_normal)
    assert same_bits(r["moments"], mm) and r["history_len"].max() == 1  # after a reset M' = M
    plain = TemporalAccumulator(0, w, h)
    assert _status(lambda: plain.accumulate(frame, g, cam, moments=True, **kw)) == abi.RT_ERR_INVALID
    assert "RT_TEMPORAL_MOMENTS" in rtlib.rt_last_error().decode()
    assert _status(lambda: plain.accumulate_moments_device(cam, 1, 1, 1, 1, 1, d_out_f32=1, **kw)) == abi.RT_ERR_INVALID
    h2 = C.c_void_p()
    assert rtlib.rt_temporal_create_ex(0, w, h, 2, C.byref(h2)) == abi.RT_ERR_INVALID and not h2.value
    for a in (host, dev, plain):
        a.close()


# ---- the variance estimate -----------------------------------------------------------------------------------------------------------------
SIG = dict(sigma_normal=0.25, sigma_position=0.4, sigma_albedo=0.1)


def test_variance_equals_the_model_with_and_without_moments_and_around_min_history(rtlib, scene_cache):
    import torch
    w, h = 64, 36
    sd = scene_cache("atrium")
    seq, scale = render_sequence(sd, w, h, 8)
    acc = TemporalAccumulator(0, w, h, moments=True)
    for frame, g, cam in seq:
        r = acc.accumulate(frame, g, cam, want_u8=False, scene_scale=scale)
    acc.close()
    n = r["history_len"]
    assert n.max() == 8 and (n < 4).any() and (n >= 4).any()  # the default min_history has data on both sides
    den = Denoiser(0, w, h, variance=True)
    sig = dict(SIG, sigma_position=float(f32(0.05) * f32(scale)))
    model_args = (sig["sigma_normal"], sig["sigma_position"], sig["sigma_albedo"])
    still = den.estimate_variance(r["f32"], g, **sig)
    assert same_bits(still, variance_model(r["f32"], g, *model_args))
    assert (still > 0).mean() > 0.5
    for mh in (0, 1, DENOISE_MIN_HISTORY, 8, 9, 2**32 - 1):
        v = den.estimate_variance(r["f32"], g, r["moments"], n, min_history=mh, **sig)
        mv = variance_model(r["f32"], g, *model_args, r["moments"], n, mh)
        assert same_bits(v, mv), (mh, np.argwhere(v.view(np.uint32) != mv.view(np.uint32))[:4])
        if mh >= 9:
            assert same_bits(v, still)
    # other sigmas, terms switched off
    for s3 in ((INF, 0.4, 0.1), (0.25, INF, 0.1), (0.25, 0.4, INF), (INF, INF, INF), (1e-3, 1e-6, 1e9)):
        kw = dict(zip(("sigma_normal", "sigma_position", "sigma_albedo"), s3))
        assert same_bits(den.estimate_variance(r["f32"], g, r["moments"], n, **kw), variance_model(r["f32"], g, *s3, r["moments"], n, 4)), s3
    # the _device form on a stream of its own
    planes = [torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (r["f32"], g["albedo"], g["normal"], g["position"], r["moments"], n)]
    dv = torch.zeros((h, w), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=0)
    den.estimate_variance_device(*(x.data_ptr() for x in planes), dv.data_ptr(), stream=st.cuda_stream, **sig)
    st.synchronize()
    assert same_bits(dv.cpu().numpy(), variance_model(r["f32"], g, *model_args, r["moments"], n, DENOISE_MIN_HISTORY))
    den.estimate_variance_device(*(x.data_ptr() for x in planes[:4]), 0, 0, dv.data_ptr(), stream=st.cuda_stream, **sig)
    st.synchronize()
    assert same_bits(dv.cpu().numpy(), still)
    den.close()


@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (65, 3)])
def test_variance_on_partial_tiles_and_an_all_miss_frame(rtlib, scene_cache, w, h):
    den = Denoiser(0, w, h, variance=True)
    frame, g, _ = _synthetic(h, w, 31)
    assert same_bits(den.estimate_variance(frame, g, **SIG), variance_model(frame, g, SIG["sigma_normal"], SIG["sigma_position"], SIG["sigma_albedo"]))
    sd = scene_cache("empty")
    s = Scene(sd, device=0)
    cam = Camera.for_scene(sd, (w, h))
    sky = _synthetic(h, w, 32)[0]  # (any frame: the estimate reads its luminance, and every pixel's kind from the guides)
    ge = s.gbuffer(cam)
    assert np.isinf(ge["position"][..., 3]).all()
    v = den.estimate_variance(sky, ge, **SIG)
    assert same_bits(v, variance_model(sky, ge, SIG["sigma_normal"], SIG["sigma_position"], SIG["sigma_albedo"]))
    mom = np.zeros((h, w, 2), f32)
    v0 = den.estimate_variance(sky, ge, mom, np.zeros((h, w), f32), **SIG)  # misses have no history: the window, among the misses
    assert same_bits(v0, v)
    s.close(), den.close()


# ---- the guided filter ---------------------------------------------------------------------------------------------------------------------
GSIG = [(4.0, 0.3, 0.4, 0.2), (INF, 0.3, 0.4, 0.2), (1.0, INF, INF, INF), (8.0, 1e-6, 1e9, 2.0)]
GNAMES = ("sigma_luminance", "sigma_normal", "sigma_position", "sigma_albedo")


@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (65, 3), (320, 180)])
def test_guided_equals_the_model(rtlib, w, h):
    den = Denoiser(0, w, h, variance=True)
    for it in (0, 1, 5, 10):
        for si, sig in enumerate(GSIG if (w, h) == (7, 5) else GSIG[:2]):
            frame, g, var = _synthetic(h, w, 100 * it + si)
            f, b, ov = den.denoise_guided(frame, g, var, iterations=it, **dict(zip(GNAMES, sig)))
            mf, mb, mv = guided_model(frame, g, var, it, *sig)
            assert same_bits(f, mf), (w, h, it, sig, np.argwhere(f.view(np.uint32) != mf.view(np.uint32))[:4])
            assert same_bits(b, mb), (w, h, it, sig)
            assert same_bits(ov, mv), (w, h, it, sig, np.argwhere(ov.view(np.uint32) != mv.view(np.uint32))[:4])
    den.close()


def test_guided_without_the_luminance_term_is_the_devices_own_rt_denoise(rtlib):
    h, w = 45, 131
    frame, g, var = _synthetic(h, w, 12)
    den = Denoiser(0, w, h, variance=True)
    for it in (0, 1, 4):
        a, ab, _ = den.denoise_guided(frame, g, var, iterations=it, sigma_luminance=INF, sigma_normal=0.3, sigma_position=0.4, sigma_albedo=0.2)
        b, bb = den.denoise(frame, g, iterations=it, sigma_color=INF, sigma_normal=0.3, sigma_position=0.4, sigma_albedo=0.2)
        assert same_bits(a, b) and same_bits(ab, bb), it
    den.close()


def test_guided_in_place_single_outputs_and_device_streams(rtlib):
    import torch
    h, w = 45, 131
    frame, g, var = _synthetic(h, w, 11)
    den = Denoiser(0, w, h, variance=True)
    sig = dict(zip(GNAMES, GSIG[0]))
    for it in (0, 1, 3):
        ref_f, ref_b, ref_v = den.denoise_guided(frame, g, var, iterations=it, **sig)
        f_only, none_b, none_v = den.denoise_guided(frame, g, var, iterations=it, want_u8=False, want_variance=False, **sig)
        none_f, b_only, _ = den.denoise_guided(frame, g, var, iterations=it, want_f32=False, **sig)
        assert none_b is None and none_v is None and none_f is None and same_bits(f_only, ref_f) and same_bits(b_only, ref_b)
        inplace = frame.copy()
        den.denoise_guided(inplace, g, var, iterations=it, out_f32=inplace, **sig)
        assert same_bits(inplace, ref_f), it
        dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in g.items()}
        df, dvar = torch.from_numpy(frame).to("cuda:0"), torch.from_numpy(var).to("cuda:0")
        du8 = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
        dov = torch.zeros((h, w), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        st = torch.cuda.Stream(device=0)
        den.denoise_guided_device(df.data_ptr(), dev["albedo"].data_ptr(), dev["normal"].data_ptr(), dev["position"].data_ptr(), dvar.data_ptr(),
                                  df.data_ptr(), du8.data_ptr(), dov.data_ptr(), stream=st.cuda_stream, iterations=it, **sig)  # in place
        st.synchronize()
        assert same_bits(df.cpu().numpy(), ref_f) and same_bits(du8.cpu().numpy(), ref_b) and same_bits(dov.cpu().numpy(), ref_v), it
    den.close()


def test_three_entry_points_on_two_streams_and_the_host_share_one_bracket(rtlib):
    """One denoiser, no host synchronisation between the calls: the estimate on stream A, the guided filter at 2 iterations on stream B reading
    that variance, then the host rt_denoise at 1 iteration. Each call's stream waits for the event behind the call before it (the estimate's
    output before the filter reads it, the scratch and staging planes before the next call writes them). 65 x 5: a full tile column and a
    one-pixel one, a full tile row and a one-row one."""
    import torch
    h, w = 5, 65
    frame, g, _ = _synthetic(h, w, 41)
    sig = dict(zip(GNAMES, GSIG[0]))
    den = Denoiser(0, w, h, variance=True)
    df, da, dn, dp = (torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (frame, g["albedo"], g["normal"], g["position"]))
    dvar = torch.zeros((h, w), dtype=torch.float32, device="cuda:0")
    dof = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    du8 = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
    dov = torch.zeros((h, w), dtype=torch.float32, device="cuda:0")
    sa, sb = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    den.estimate_variance_device(df.data_ptr(), da.data_ptr(), dn.data_ptr(), dp.data_ptr(), 0, 0, dvar.data_ptr(), stream=sa.cuda_stream, **SIG)
    den.denoise_guided_device(df.data_ptr(), da.data_ptr(), dn.data_ptr(), dp.data_ptr(), dvar.data_ptr(), dof.data_ptr(), du8.data_ptr(),
                              dov.data_ptr(), stream=sb.cuda_stream, iterations=2, **sig)
    hf, hb = den.denoise(frame, g, iterations=1, sigma_color=0.7, sigma_normal=0.3, sigma_position=0.4, sigma_albedo=0.2)
    torch.cuda.synchronize()
    mv = variance_model(frame, g, SIG["sigma_normal"], SIG["sigma_position"], SIG["sigma_albedo"])
    assert same_bits(dvar.cpu().numpy(), mv)
    mf, mb, mov = guided_model(frame, g, mv, 2, *GSIG[0])
    assert same_bits(dof.cpu().numpy(), mf) and same_bits(du8.cpu().numpy(), mb) and same_bits(dov.cpu().numpy(), mov)
    df1, db1 = _m._dn.denoise_model(frame, g, 1, 0.7, 0.3, 0.4, 0.2)
    assert same_bits(hf, df1) and same_bits(hb, db1)
    den.close()


def test_guided_at_the_contracts_edges(rtlib):
    """Zero variance everywhere; one 1e20 firefly (include/rt_mi355x.h, "Non-finite radiance"); a hit / miss checkerboard."""
    h, w = 40, 70
    den = Denoiser(0, w, h, variance=True)
    sig = dict(zip(GNAMES, GSIG[0]))
    frame, g, var = _synthetic(h, w, 21)
    zero = np.zeros((h, w), f32)
    for it in (1, 3):
        f, b, ov = den.denoise_guided(frame, g, zero, iterations=it, **sig)
        mf, mb, mv = guided_model(frame, g, zero, it, *GSIG[0])
        assert same_bits(f, mf) and same_bits(b, mb) and same_bits(ov, mv) and (ov == 0).all(), it
    # the firefly: through the estimate and the filter, against the models and against the header's statement
    g["position"][..., 3] = 1.0
    fire = frame.copy()
    fire[20, 33, :3] = 1e20
    v = den.estimate_variance(fire, g, **SIG)
    mv = variance_model(fire, g, SIG["sigma_normal"], SIG["sigma_position"], SIG["sigma_albedo"])
    assert same_bits(v, mv) and not np.isnan(v).any()
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    # (the window's weights may be 0 for unlike guides: where the firefly's weight is not, m1 and m2 are +inf and the variance is 0)
    assert v[20, 33] == 0
    for it in (1, 2):
        f, b, ov = den.denoise_guided(fire, g, v, iterations=it, **sig)
        mf, mb, mov = guided_model(fire, g, v, it, *GSIG[0])
        assert same_bits_or_nan(f, mf) and same_bits_or_nan(ov, mov), it
        finite = ~np.isnan(mf[..., :3]).any(-1)
        assert same_bits(b[finite], mb[finite]), it
        assert np.isnan(f[20, 33, 0]) and np.isnan(ov[20, 33]) and np.isfinite(f[0, 0]).all()
    one = den.denoise_guided(fire, g, v, iterations=1, **sig)
    assert np.array_equal(np.isnan(one[0][..., 0]), (abs(ys - 20) <= 2) & (abs(xs - 33) <= 2))
    assert np.array_equal(np.isnan(one[2]), (ys == 20) & (xs == 33))
    # the checkerboard: hits and misses never mix
    frame, g, var = _synthetic(h, w, 22)
    miss = (ys + xs) % 2 == 0
    g["position"][..., 3] = 1.0
    g["position"][miss] = (0, 0, 0, np.inf)
    frame[miss, :3] = 1.0
    frame[~miss, :3] = 0.25
    for it in (1, 2, 5):
        f, b, ov = den.denoise_guided(frame, g, var, iterations=it, sigma_luminance=4.0, sigma_normal=INF, sigma_position=INF, sigma_albedo=INF)
        mf, mb, mov = guided_model(frame, g, var, it, 4.0, INF, INF, INF)
        assert same_bits(f, mf) and same_bits(b, mb) and same_bits(ov, mov), it
        assert np.allclose(f[miss, :3], 1.0, rtol=1e-6) and np.allclose(f[~miss, :3], 0.25, rtol=1e-6)
    vc = den.estimate_variance(frame, g, **SIG)
    assert same_bits(vc, variance_model(frame, g, SIG["sigma_normal"], SIG["sigma_position"], SIG["sigma_albedo"])) and np.allclose(vc, 0, atol=1e-6)
    den.close()


def test_refusals_with_live_handles(rtlib):
    h, w = 4, 5
    frame, g, var = _synthetic(h, w, 1)
    den, plain = Denoiser(0, w, h, variance=True), Denoiser(0, w, h)
    ok = dict(zip(GNAMES, (4.0, 1.0, 1.0, 1.0)))
    assert _status(lambda: plain.denoise_guided(frame, g, var, iterations=1, **ok)) == abi.RT_ERR_INVALID
    assert "RT_DENOISER_VARIANCE" in rtlib.rt_last_error().decode()
    assert _status(lambda: plain.estimate_variance(frame, g, **ok)) == abi.RT_ERR_INVALID
    assert _status(lambda: plain.denoise_guided_device(1, 1, 1, 1, 1, 1, iterations=1, **ok)) == abi.RT_ERR_INVALID
    assert _status(lambda: plain.estimate_variance_device(1, 1, 1, 1, 0, 0, 1, **ok)) == abi.RT_ERR_INVALID
    plain.denoise(frame, g, iterations=1, sigma_color=1.0, sigma_normal=1.0, sigma_position=1.0, sigma_albedo=1.0)  # ... and still denoises
    den.denoise(frame, g, iterations=1, sigma_color=1.0, sigma_normal=1.0, sigma_position=1.0, sigma_albedo=1.0)    # as a flagged one does
    assert _status(lambda: den.denoise_guided(frame, g, var, iterations=11, **ok)) == abi.RT_ERR_INVALID
    for bad in (0.0, 1e-7, -1.0, float("nan")):
        for name in ok:
            assert _status(lambda: den.denoise_guided(frame, g, var, iterations=1, **dict(ok, **{name: bad}))) == abi.RT_ERR_INVALID, (name, bad)
            assert _status(lambda: den.estimate_variance(frame, g, **dict(ok, **{name: bad}))) == abi.RT_ERR_INVALID, (name, bad)
    assert _status(lambda: den.denoise_guided(frame, g, var, iterations=1, want_f32=False, want_u8=False, **ok)) == abi.RT_ERR_INVALID
    assert _status(lambda: den.estimate_variance(frame, g, np.zeros((h, w, 2), f32), None, **ok)) == abi.RT_ERR_INVALID
    p = denoise_var_params(1, **ok)
    assert den._lib.rt_denoise_guided_device(den.h, C.byref(p), 1, 1, 1, 1, None, 1, None, None, None) == abi.RT_ERR_INVALID
    assert den._lib.rt_denoise_variance_device(den.h, C.byref(p), 1, 1, 1, 1, None, None, None, None) == abi.RT_ERR_INVALID
    h2 = C.c_void_p()
    assert rtlib.rt_denoiser_create_ex(0, w, h, 4, C.byref(h2)) == abi.RT_ERR_INVALID and not h2.value
    den.close(), plain.close()


# ---- the CLI -------------------------------------------------------------------------------------------------------------------------------
def _masked(stdout):
    return [re.sub(r"\d+\.\d+", "#", ln) for ln in stdout.splitlines()]


def test_cli_guided_still_writes_the_python_path_image_and_leaves_plain_denoise_alone(rtlib, scene_cache, tmp_path):
    from PIL import Image
    from rtamd import loader
    sd = scene_cache("cornell")
    glb = tmp_path / "cornell.glb"
    export_glb(sd, glb)
    w, h, depth, spp = 96, 72, 6, 4
    base = [str(EXE), "-w", "-d", str(depth), "-s", str(spp), "--width", str(w), "--height", str(h), "--quiet", "--denoise", "5"]
    p = subprocess.run([*base, "--guided", "4", "--out", str(tmp_path / "g.png"), str(glb)], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    assert re.search(r"^Denoise: 5 iterations, G-buffer \d+\.\d+ ms, variance \d+\.\d+ ms, filter \d+\.\d+ ms on device 0$", p.stdout, re.M), p.stdout
    q = subprocess.run([*base, "--out", str(tmp_path / "d.png"), str(glb)], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert q.returncode == 0, q.stdout + q.stderr
    # without --guided: the lines of every run before this option existed, and rt_denoise's image
    assert re.search(r"^Denoise: 5 iterations, G-buffer \d+\.\d+ ms, filter \d+\.\d+ ms on device 0$", q.stdout, re.M), q.stdout
    assert "variance" not in q.stdout
    assert [ln for ln in _masked(p.stdout) if not ln.startswith("Denoise:")] == [ln for ln in _masked(q.stdout) if not ln.startswith("Denoise:")]
    ld = loader.load_glb(glb)
    s = Scene(ld, device=0)
    cam = Camera((w, h), ld.camera.position, ld.camera.direction, ld.camera.focal_length)
    frame = WavefrontRenderer(s, (w, h), depth, spp).render_frame(cam).rgba_f32
    g = s.gbuffer(cam)
    den = Denoiser(0, w, h, variance=True)
    _, plain_u8 = den.denoise(frame, g, iterations=5, scene_scale=s.scale())
    assert same_bits(np.asarray(Image.open(tmp_path / "d.png")), plain_u8)
    var = den.estimate_variance(frame, g, scene_scale=s.scale())
    _, u8, _ = den.denoise_guided(frame, g, var, iterations=5, sigma_luminance=4.0, scene_scale=s.scale())
    assert same_bits(np.asarray(Image.open(tmp_path / "g.png")), u8)
    assert not same_bits(u8, plain_u8)
    # a tiled frame (two tiles, gathered on the root) is filtered there to the same image
    t = subprocess.run([*base, "--guided", "4", "--devices", "0,0", "--out", str(tmp_path / "t.png"), str(glb)], capture_output=True, text=True,
                       timeout=300, cwd=tmp_path)
    assert t.returncode == 0, t.stdout + t.stderr
    assert same_bits(np.asarray(Image.open(tmp_path / "t.png")), u8)
    bad = subprocess.run([str(EXE), "--guided", "4", str(glb)], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 105 and "--guided" in bad.stderr and "--denoise" in bad.stderr
    den.close(), s.close()


def test_cli_guided_over_a_temporal_sequence_writes_the_python_path_images(rtlib, tmp_path):
    from PIL import Image
    from rtamd import loader
    cli_spin = _load("test_gpu_temporal").cli_spin
    glb = REPO / "assets" / "cube.glb"
    w, h, depth, spp, frames, spin, hist = 96, 72, 6, 2, 4, 2.0, 8
    base = [str(EXE), "-w", "-d", str(depth), "-s", str(spp), "--width", str(w), "--height", str(h), "--quiet", "--frames", str(frames),
            "--spin", str(spin), "--temporal", str(hist), "--denoise", "5"]
    p = subprocess.run([*base, "--guided", "4", "--out", str(tmp_path / "g.png"), str(glb)], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    assert len(re.findall(r"^Denoise: 5 iterations, G-buffer \S+ ms, variance \S+ ms, filter \S+ ms on device 0$", p.stdout, re.M)) == frames, p.stdout
    q = subprocess.run([*base, "--out", str(tmp_path / "d.png"), str(glb)], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert q.returncode == 0, q.stdout + q.stderr
    assert len(re.findall(r"^Denoise: 5 iterations, G-buffer \S+ ms, filter \S+ ms on device 0$", q.stdout, re.M)) == frames and "variance" not in q.stdout
    assert [ln for ln in _masked(p.stdout) if not ln.startswith("Denoise:")] == [ln for ln in _masked(q.stdout) if not ln.startswith("Denoise:")]
    ld = loader.load_glb(glb)
    cam = Camera((w, h), ld.camera.position, ld.camera.direction, ld.camera.focal_length)
    s = Scene(ld, device=0, updatable=True, keep_previous=True)
    i = s.info()
    centre = [f32(0.5) * (f32(i.bounds_lo[k]) + f32(i.bounds_hi[k])) for k in range(3)]
    r = WavefrontRenderer(s, (w, h), depth, spp)
    acc, plain_acc = TemporalAccumulator(0, w, h, moments=True), TemporalAccumulator(0, w, h)
    den = Denoiser(0, w, h, variance=True)
    for f in range(frames):
        if f:
            s.update(instances=cli_spin(ld, centre, spin * f))
        r.set_frame_seed(f)
        fr = r.render_frame(cam).rgba_f32
        gm = s.gbuffer_motion(cam)
        a = acc.accumulate(fr, gm, cam, max_history=hist, scene_scale=s.scale())
        var = den.estimate_variance(a["f32"], gm, a["moments"], a["history_len"], scene_scale=s.scale())
        _, u8, _ = den.denoise_guided(a["f32"], gm, var, iterations=5, sigma_luminance=4.0, scene_scale=s.scale())
        assert same_bits(np.asarray(Image.open(tmp_path / f"g_{f:04d}.png")), u8), f
        po, _, _ = plain_acc.accumulate(fr, gm, cam, max_history=hist, scene_scale=s.scale())
        _, pu8 = den.denoise(po, gm, iterations=5, scene_scale=s.scale())
        assert same_bits(np.asarray(Image.open(tmp_path / f"d_{f:04d}.png")), pu8), f  # without --guided: the images it always wrote
    for x in (acc, plain_acc, den, r, s):
        x.close()


# ---- quality (reported, as DESIGN.md §15's) ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["atrium", "cornell"])
def test_quality_of_the_guided_chain_is_reported(rtlib, scene_cache, name):
    """16 frames at 4 spp, salts 1 .. 16, 1 degree per frame, 320 x 180, against a 1024-spp frame of the final scene state, linear radiance:
    the still (last raw frame) and the accumulated frame, each through rt_denoise and through the guided chain at the defaults. Reported; the
    one assertion is that the guided chain runs and returns numbers."""
    sd0 = scene_cache(name)
    w, h, depth, spp, n_frames = 320, 180, 10, 4, 16
    s = Scene(sd0, device=0, updatable=True, keep_previous=True)
    cam = Camera.for_scene(sd0, (w, h))
    r = MegakernelRenderer(s, (w, h), depth, spp)
    acc = TemporalAccumulator(0, w, h, moments=True)
    for f in range(n_frames):
        if f:
            s.update(instances=spin_about_centre(sd0, 1.0 * f))
        r.set_frame_seed(f + 1)
        raw = r.render_frame(cam, want_u8=False).rgba_f32
        g = s.gbuffer_motion(cam)
        a = acc.accumulate(raw, g, cam, want_u8=False, scene_scale=s.scale())
    ref = MegakernelRenderer(s, (w, h), depth, 1024).render_frame(cam, want_u8=False).rgba_f32
    den = Denoiser(0, w, h, variance=True)
    sc = s.scale()
    e = {"raw": raw, "temporal": a["f32"]}
    e["raw+atrous"], _ = den.denoise(raw, g, want_u8=False, scene_scale=sc)
    e["temporal+atrous"], _ = den.denoise(a["f32"], g, want_u8=False, scene_scale=sc)
    e["raw+guided"], _, _ = den.denoise_guided(raw, g, den.estimate_variance(raw, g, scene_scale=sc), want_u8=False, scene_scale=sc)
    tv = den.estimate_variance(a["f32"], g, a["moments"], a["history_len"], scene_scale=sc)
    e["temporal+guided"], _, _ = den.denoise_guided(a["f32"], g, tv, want_u8=False, scene_scale=sc)
    e = {k: linear_rmse(v, ref) for k, v in e.items()}
    print(f"\nquality 320x180 {name}, 16 frames x 4 spp, 1 degree per frame, sigma_luminance {DENOISE_SIGMA_LUMINANCE}: " +
          ", ".join(f"{k} {v:.6f}" for k, v in e.items()))
    assert all(np.isfinite(v) for v in e.values())
    s.close()
