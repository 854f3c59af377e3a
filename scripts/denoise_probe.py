"""Cost and quality of the G-buffer and the a-trous denoiser -> profiles/denoise_probe.json.

Cost: rt_scene_gbuffer_device and rt_denoise_device of the 1920x1080 atrium, hipEvents on one stream, the median of 20 runs after 3 warm-up runs.
Usage: python scripts/denoise_probe.py [OUT.json]
Quality: the RMSE of the linear image (squared fp32 frame) against a 1024-spp frame, raw and denoised (the default sigmas), at 1, 4, 8 and 16 spp
on the atrium and the Cornell box at 320x180, and a small sweep of the sigmas on the 4-spp frames."""
import itertools
import json
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "sycl-ray-tracer_amd"))
from rtamd import renderer as R  # noqa: E402
from rtamd import scenes  # noqa: E402


def timed(fn, runs=20, warm=3):
    st = torch.cuda.Stream(device=0)
    ms = []
    for i in range(warm + runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(st):
            a.record(st)
            fn(st.cuda_stream)
            b.record(st)
        b.synchronize()
        if i >= warm:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), [float(x) for x in ms]


def rmse(a, ref):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) ** 2 - ref[..., :3].astype(np.float64) ** 2) ** 2)))


def main():
    out = {}
    sd = scenes.get_scene("atrium")
    s = R.Scene(sd, device=0)
    w, h = 1920, 1080
    cam = R.Camera.for_scene(sd, (w, h))
    planes = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    g_ms, g_all = timed(lambda st: s.gbuffer_device(cam, *(p.data_ptr() for p in planes), stream=st))
    frame = torch.from_numpy(R.WavefrontRenderer(s, (w, h), 10, 8).render_frame(cam, want_u8=False).rgba_f32).to("cuda:0")
    outf = torch.zeros_like(frame)
    outb = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
    d = R.Denoiser(0, w, h)
    cost = {"gbuffer_ms": g_ms, "gbuffer_runs_ms": g_all}
    for it in (1, 3, 5):
        ms, allms = timed(lambda st: d.denoise_device(frame.data_ptr(), *(p.data_ptr() for p in planes), outf.data_ptr(), outb.data_ptr(),
                                                      stream=st, iterations=it, scene_scale=s.scale()))
        cost[f"denoise_{it}_ms"] = ms
        cost[f"denoise_{it}_per_iteration_ms"] = ms / it
        cost[f"denoise_{it}_runs_ms"] = allms
    out["atrium_1920x1080"] = cost
    print(json.dumps({k: v for k, v in cost.items() if not k.endswith("runs_ms")}), flush=True)
    s.close()

    quality, sweep = {}, {}
    for name in ("atrium", "cornell"):
        sd = scenes.get_scene(name)
        s = R.Scene(sd, device=0)
        w, h = 320, 180
        cam = R.Camera.for_scene(sd, (w, h))
        ref = R.MegakernelRenderer(s, (w, h), 10, 1024).render_frame(cam, want_u8=False).rgba_f32
        g = s.gbuffer(cam)
        d = R.Denoiser(0, w, h)
        rows = {}
        frames = {}
        for spp in (1, 4, 8, 16, 64):
            f = R.MegakernelRenderer(s, (w, h), 10, spp).render_frame(cam, want_u8=False).rgba_f32
            frames[spp] = f
            row = {"raw": rmse(f, ref)}
            if spp <= 16:
                den, _ = d.denoise(f, g, scene_scale=s.scale())
                row["denoised"] = rmse(den, ref)
            rows[spp] = row
        quality[name] = rows
        grid = {}
        for sc, sn, fp, sa in itertools.product((0.5, 1.0, 2.0, float("inf")), (0.25, 1.0), (0.02, 0.05, 0.2), (0.1, float("inf"))):
            den, _ = d.denoise(frames[4], g, iterations=5, sigma_color=sc, sigma_normal=sn, sigma_position=float(np.float32(fp) * s.scale()),
                               sigma_albedo=sa)
            grid[f"c={sc} n={sn} xfrac={fp} a={sa}"] = rmse(den, ref)
        sweep[name] = dict(sorted(grid.items(), key=lambda kv: kv[1])[:8])
        print(name, json.dumps(rows), json.dumps(sweep[name]), flush=True)
        s.close()
    out["quality_rmse_linear_vs_1024spp_320x180"] = quality
    out["sweep_4spp_best8"] = sweep
    out["defaults"] = dict(iterations=R.DENOISE_ITERATIONS, sigma_color=R.DENOISE_SIGMA_COLOR, sigma_normal=R.DENOISE_SIGMA_NORMAL,
                           position_fraction=R.DENOISE_POSITION_FRACTION, sigma_albedo=R.DENOISE_SIGMA_ALBEDO)
    dst = Path(sys.argv[1]) if len(sys.argv) > 1 else REPO / "profiles" / "denoise_probe.json"
    dst.parent.mkdir(parents=True, exist_ok=True)
    dst.write_text(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
