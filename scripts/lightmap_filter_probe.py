"""Cost and quality of the lightmap filter -> profiles/lightmap_filter_probe.json.

    python scripts/lightmap_filter_probe.py [profiles/lightmap_filter_probe.json]

One process, hipEvents on one stream, 3 warm-up and 20 timed runs per window: median, min and max. The two atlases of §19:
  atrium_4096   the detail-4 atrium on 4096 x 4096, cells of 7 texels with a gutter of 1
  coarse_1024   the coarse atrium (235,750 triangles) on 1024 x 1024, cells of 2 texels without a gutter
Cost, per atlas: rt_lightmap_bake_device and rt_lightmap_bake_filtered_device with 0, 1 and 5 iterations at 4 samples x 4 repeats, depth 10;
rt_lightmap_filter_device alone on that bake's planes with 0, 1, 2 and 5 iterations (no gather in the window, so the differences of medians
are not held against a 75 ms gather's spread); the same five-iteration window from the developer build with and without the early exit of
texels outside the mask (RT_LM_FILTER_NO_EARLY_EXIT); and rt_denoise_guided_device at the same texel count with 1 and 5 iterations, every
pixel a hit, all four sigmas finite. Per-iteration times are differences of medians.
Quality, per atlas: RMSE over the sampled texels against a bake of 256 samples x 4 repeats (1,024 paths per texel, another seed) of the raw
4 x 4 bake and of the filtered one, at the Python defaults and over a sweep of sigma_luminance and the position fraction.
The bound of tests/test_gpu_lightmap_filter.py's quality test: the Cornell box under the grid unwrap on 256 x 256, depth 5, the ratio
filtered / raw at the defaults for eight seeds, the largest times 1.25; and the sweep there over all eight seeds.
No pass mark: the figures are reported as they are."""
import json
import os
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "sycl-ray-tracer_amd"))
from rtamd import abi, bake, scenes  # noqa: E402
from rtamd import renderer as R  # noqa: E402

DEPTH, SAMPLES, REPEATS, SEED = 10, 4, 4, 7
REF_SAMPLES, REF_SEED = 256, 1001
WARM, RUNS = 3, 20
SWEEP_L, SWEEP_X = (2.0, 4.0, 8.0), (0.025, 0.05, 0.1)
f32 = np.float32


def timed(fn):
    import torch
    ms = []
    for k in range(WARM + RUNS):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k >= WARM:
            ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "runs": RUNS}


def rmse(a, ref, on):
    import torch
    d = (a[:, :3] - ref[:, :3])[on].double()
    return float(torch.sqrt((d * d).mean()).item())


def defaults(scale):
    return dict(iterations=R.LIGHTMAP_FILTER_ITERATIONS, sigma_luminance=R.LIGHTMAP_SIGMA_LUMINANCE, sigma_normal=R.LIGHTMAP_SIGMA_NORMAL,
                sigma_position=float(f32(R.LIGHTMAP_POSITION_FRACTION) * f32(scale)))


def sweep(bake_filtered, raw_rmse, ref, on, scale, out):
    """filtered / raw over SWEEP_L x SWEEP_X at the default iterations and sigma_normal"""
    rows = []
    for sl in SWEEP_L:
        for fx in SWEEP_X:
            kw = dict(defaults(scale), sigma_luminance=sl, sigma_position=float(f32(fx) * f32(scale)))
            bake_filtered(kw)
            e = rmse(out, ref, on)
            rows.append({"sigma_luminance": sl, "position_fraction": fx, "rmse": e, "ratio": e / raw_rmse})
    return rows


def atlas_case(sd, size, gutter):
    import torch
    s = R.Scene(sd, device=0)
    scale = s.scale()
    stream = torch.cuda.current_stream().cuda_stream
    n = size * size
    uv = bake.triangle_grid_uvs(sd.n_triangles, size, size, gutter)
    lm = R.Lightmap(s, uv, size, size, max_repeats=REPEATS, filter=True)
    rgba, out, ref = (torch.empty((n, 4), dtype=torch.float32, device="cuda") for _ in range(3))
    var, ovar = (torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(2))
    stats = torch.zeros(3, dtype=torch.int64, device="cuda")
    dflt = defaults(scale)

    def filtered(kw, dst=out):
        lm.bake_filtered_device(dst.data_ptr(), SAMPLES, DEPTH, SEED, repeats=REPEATS, d_variance=ovar.data_ptr(), d_stats=stats.data_ptr(),
                                stream=stream, **kw)

    def filter_only(lmx, it):
        return lambda: lmx.filter_device(rgba.data_ptr(), var.data_ptr(), out.data_ptr(), ovar.data_ptr(), stream=stream, **dict(dflt, iterations=it))

    res = {"atlas": size, "gutter": gutter, "triangles": sd.n_triangles, "texels": n, "scene_scale": float(scale), "defaults": dflt}
    res["bake"] = timed(lambda: lm.bake_device(out.data_ptr(), SAMPLES, DEPTH, SEED, repeats=REPEATS, stream=stream))
    for it in (0, 1, 5):
        res[f"bake_filtered_{it}"] = timed(lambda: filtered(dict(dflt, iterations=it)))
    # the raw planes the filter-only windows and the image filter read: the unfiltered bake and the variance of its mean
    lm.bake_filtered_device(rgba.data_ptr(), SAMPLES, DEPTH, SEED, repeats=REPEATS, d_variance=var.data_ptr(), d_stats=stats.data_ptr(),
                            stream=stream, **dict(dflt, iterations=0))
    torch.cuda.synchronize()
    w = stats.cpu().numpy()
    res["stats"] = {"covered": int(w.view(np.uint32)[0]), "sampled": int(w.view(np.uint32)[1]), "rays": int(w.view(np.uint64)[2])}
    m = res["stats"]["sampled"]
    for it in (0, 1, 2, 5):
        res[f"filter_{it}"] = timed(filter_only(lm, it))
    b0, b1, b5 = (res[f"bake_filtered_{k}"]["median_ms"] for k in (0, 1, 5))
    f0, f1, f2, f5 = (res[f"filter_{k}"]["median_ms"] for k in (0, 1, 2, 5))
    res["derived_ms"] = {"bake_filtered_0_minus_bake": b0 - res["bake"]["median_ms"], "bake_first_iteration": b1 - b0,
                         "bake_iteration_mean_of_2_to_5": (b5 - b1) / 4, "filter_first_iteration": f1 - f0, "filter_second_iteration": f2 - f1,
                         "filter_iteration_mean_of_2_to_5": (f5 - f1) / 4, "filter_iteration_mean_of_5": (f5 - f0) / 5}
    per = res["derived_ms"]["filter_iteration_mean_of_5"]
    res["ns_per_texel_in_mask_per_iteration"] = per * 1e6 / m
    res["ns_per_atlas_texel_per_iteration"] = per * 1e6 / n
    # bytes one texel in M moves per iteration where every tap beside its own hits a cache: colour + two guide planes in, colour out
    res["bytes_per_texel_unique"] = {"lightmap_iteration": 16 + 16 + 16 + 16, "image_iteration": 16 + 16 + 16 + 16 + 16}

    # the early exit, both ways, in the developer build (the one build that reads the knob)
    dev = abi.load_developer_library()
    sdev = R.Scene(sd, device=0, lib=dev)
    lmd = R.Lightmap(sdev, uv, size, size, max_repeats=1, filter=True)
    res["dev_filter_5_early_exit"] = timed(filter_only(lmd, 5))
    os.environ["RT_LM_FILTER_NO_EARLY_EXIT"] = "1"
    res["dev_filter_5_no_early_exit"] = timed(filter_only(lmd, 5))
    del os.environ["RT_LM_FILTER_NO_EARLY_EXIT"]
    res["dev_filter_5_early_exit_again"] = timed(filter_only(lmd, 5))
    lmd.close(), sdev.close()

    # k_atrous_guided at the same texel count: the lightmap's guides as float4 planes with a finite .w (every pixel a hit), a random albedo
    pos, nrm = (torch.empty((n, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    lm.texels_device(0, pos.data_ptr(), nrm.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    one = torch.ones((n, 1), dtype=torch.float32, device="cuda")
    gpos, gnrm = torch.cat([torch.nan_to_num(pos), one], 1).contiguous(), torch.cat([nrm, one], 1).contiguous()
    alb = torch.rand((n, 4), dtype=torch.float32, device="cuda")
    del pos, nrm, one
    dn = R.Denoiser(0, size, size, variance=True)
    for it in (1, 5):
        res[f"image_guided_{it}"] = timed(lambda: dn.denoise_guided_device(rgba.data_ptr(), alb.data_ptr(), gnrm.data_ptr(), gpos.data_ptr(),
                                                                          var.data_ptr(), d_out_f32=out.data_ptr(), d_out_variance=ovar.data_ptr(),
                                                                          stream=stream, iterations=it, scene_scale=scale))
    dn.close()
    del gpos, gnrm, alb
    per_img = (res["image_guided_5"]["median_ms"] - res["image_guided_1"]["median_ms"]) / 4
    res["derived_ms"]["image_iteration_mean_of_2_to_5"] = per_img
    res["ns_per_pixel_per_image_iteration"] = per_img * 1e6 / n

    # quality
    lm.bake_device(ref.data_ptr(), REF_SAMPLES, DEPTH, REF_SEED, repeats=REPEATS, stream=stream)
    torch.cuda.synchronize()
    on = ref[:, 3] == 1
    q = {"reference_paths": REF_SAMPLES * REPEATS, "paths": SAMPLES * REPEATS, "raw_rmse": rmse(rgba, ref, on)}
    filtered(dflt)
    q["defaults_rmse"] = rmse(out, ref, on)
    q["defaults_ratio"] = q["defaults_rmse"] / q["raw_rmse"]
    q["sweep"] = sweep(filtered, q["raw_rmse"], ref, on, scale, out)
    res["quality"] = q
    lm.close(), s.close()
    return res


def cornell_bound():
    """what tests/test_gpu_lightmap_filter.py's quality test runs, for eight seeds"""
    import torch
    sd = scenes.get_scene("cornell")
    size, depth = 256, 5
    s = R.Scene(sd, device=0)
    scale = s.scale()
    lm = R.Lightmap(s, bake.triangle_grid_uvs(sd.n_triangles, size, size), size, size, max_repeats=REPEATS, filter=True)
    ref = torch.from_numpy(lm.bake(REF_SAMPLES, depth, REF_SEED, repeats=REPEATS)["rgba"].reshape(-1, 4)).cuda()
    on = ref[:, 3] == 1
    seeds = [11, 12, 13, 14, 15, 16, 17, 18]
    ratios, rows = [], {}
    for seed in seeds:
        raw = torch.from_numpy(lm.bake(SAMPLES, depth, seed, repeats=REPEATS)["rgba"].reshape(-1, 4)).cuda()
        e_raw = rmse(raw, ref, on)
        flt = torch.from_numpy(lm.bake_filtered(SAMPLES, depth, seed, repeats=REPEATS)["rgba"].reshape(-1, 4)).cuda()
        ratios.append(rmse(flt, ref, on) / e_raw)
        for it in (3, 5):
            for sl in SWEEP_L:
                for sn in (0.25, 0.5):
                    for fx in SWEEP_X:
                        f = lm.bake_filtered(SAMPLES, depth, seed, repeats=REPEATS, iterations=it, sigma_luminance=sl, sigma_normal=sn,
                                             sigma_position=float(f32(fx) * f32(scale)))
                        rows.setdefault((it, sl, sn, fx), []).append(rmse(torch.from_numpy(f["rgba"].reshape(-1, 4)).cuda(), ref, on) / e_raw)
    lm.close(), s.close()
    table = [{"iterations": k[0], "sigma_luminance": k[1], "sigma_normal": k[2], "position_fraction": k[3], "mean_ratio": float(np.mean(v)),
              "max_ratio": float(max(v))} for k, v in rows.items()]
    return {"atlas": size, "depth": depth, "sampled": int(on.sum().item()), "scene_scale": float(scale), "seeds": seeds, "ratios": ratios,
            "largest": max(ratios), "bound": 1.25 * max(ratios), "sweep": sorted(table, key=lambda r: r["mean_ratio"])}


def main(dest: Path):
    result = {"depth": DEPTH, "samples": SAMPLES, "repeats": REPEATS, "warmup": WARM, "runs": RUNS,
              "cornell_256": cornell_bound(),
              "coarse_1024": atlas_case(scenes.get_scene("atrium", coarse=True), 1024, 0),
              "atrium_4096": atlas_case(scenes.get_scene("atrium"), 4096, 1)}
    dest.parent.mkdir(parents=True, exist_ok=True)
    dest.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main(Path(sys.argv[1]) if len(sys.argv) > 1 else REPO / "profiles" / "lightmap_filter_probe.json")
