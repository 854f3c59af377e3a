"""Cost and settings of the temporal stage -> profiles/temporal_probe.json.

Cost, 1920x1080 atrium on one device: rt_scene_gbuffer_motion_device (rt_scene_gbuffer_device beside it) and rt_temporal_accumulate_device with a
static camera and scene, and after a spin of 1 degree (the taps straddle rows). A kernel of tens of microseconds is not timed singly: hipEvents
on one stream around a batch of BATCH back-to-back calls, per-call time = batch / BATCH, the median of 20 batches after 3 warm-up batches.
The snapshot's share of rt_scene_update: the update's device_ms (bench atrium, detail 4, every instance turned) with and without
RT_SCENE_KEEP_PREVIOUS, medians of 17 after 3 warm-up updates, as scripts/refit_probe.py measures it.
Settings: on the spinning atrium and Cornell box (320x180, 16 frames at 4 spp, salts 1 .. 16, 1 degree per frame) the RMSE of the last
accumulated frame in linear radiance against a 1024-spp frame of the final state, over a grid of max_history, sigma_position and cos_normal.
Usage: python scripts/temporal_probe.py [OUT.json]   (run it under a time limit: timeout -k 10 600 python scripts/temporal_probe.py)"""
import itertools
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "sycl-ray-tracer_amd"))
sys.path.insert(0, str(REPO / "tests"))
from rtamd import renderer as R  # noqa: E402
from rtamd import scenes  # noqa: E402
from test_scene_update import spin_about_centre  # noqa: E402

BATCH = 50


def timed(fn, runs=20, warm=3, batch=BATCH):
    st = torch.cuda.Stream(device=0)
    ms = []
    for i in range(warm + runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(st):
            a.record(st)
            for _ in range(batch):
                fn(st.cuda_stream)
            b.record(st)
        b.synchronize()
        if i >= warm:
            ms.append(a.elapsed_time(b) / batch)
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), batches=runs, calls_per_batch=batch)


def rmse(a, ref):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) ** 2 - ref[..., :3].astype(np.float64) ** 2) ** 2)))


def cost():
    sd = scenes.get_scene("atrium")
    s = R.Scene(sd, device=0, updatable=True, keep_previous=True)
    w, h = 1920, 1080
    cam = R.Camera.for_scene(sd, (w, h))
    planes = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0") for _ in range(4)]
    frame = torch.from_numpy(R.WavefrontRenderer(s, (w, h), 10, 4).render_frame(cam, want_u8=False).rgba_f32).to("cuda:0")
    outf = torch.zeros_like(frame)
    outb = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
    acc = R.TemporalAccumulator(0, w, h)
    out = {"pixels": w * h, "estimate_bytes_per_pixel": 180, "estimate_ms_at_6.3_TB_per_s": 180 * w * h / 6.3e12 * 1e3}
    out["gbuffer_device"] = timed(lambda st: s.gbuffer_device(cam, *(p.data_ptr() for p in planes[:3]), stream=st))
    for label, deg in (("static", 0.0), ("spin_1_degree", 1.0)):
        if deg:
            s.update(instances=spin_about_centre(sd, deg))
        out[f"gbuffer_motion_device_{label}"] = timed(lambda st: s.gbuffer_motion_device(cam, *(p.data_ptr() for p in planes), stream=st))
        torch.cuda.synchronize()
        call = lambda st: acc.accumulate_device(cam, frame.data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), planes[3].data_ptr(),  # noqa: E731
                                                outf.data_ptr(), outb.data_ptr(), 0, stream=st, scene_scale=s.scale())
        t = timed(call)
        t["GB_per_s_of_the_estimates_bytes"] = 180 * w * h / (t["median_ms"] * 1e-3) / 1e9
        n = torch.zeros((h, w), dtype=torch.float32, device="cuda:0")
        acc.accumulate_device(cam, frame.data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), planes[3].data_ptr(), outf.data_ptr(), 0, n.data_ptr(),
                              scene_scale=s.scale())
        torch.cuda.synchronize()
        t["pixels_with_history"] = float((n >= 2).float().mean().item())
        out[f"accumulate_device_{label}"] = t
    s.close()
    return out


def snapshot():
    sd = scenes.atrium_scene(4)
    out = {"scene": "atrium detail 4", "triangles": sd.n_triangles}
    for label, keep in (("updatable", False), ("keep_previous", True)):
        s = R.Scene(sd, 0, updatable=True, keep_previous=keep)
        poses = [spin_about_centre(sd, 30.0 * (k % 7 + 1) / 7.0) for k in range(20)]
        for p in poses[:3]:
            s.update(instances=p)
        dev = [s.update(instances=p).device_ms for p in poses[3:]]
        st = s.update(instances=poses[0])
        out[label] = dict(device_ms_median=statistics.median(dev), device_ms_min=min(dev), device_ms_max=max(dev), n=len(dev), launches=st.launches,
                          device_bytes=s.info().device_bytes)
        s.close()
    out["snapshot_share_ms"] = out["keep_previous"]["device_ms_median"] - out["updatable"]["device_ms_median"]
    return out


def sweep(name):
    sd0 = scenes.get_scene(name)
    w, h, depth, spp, n_frames = 320, 180, 10, 4, 16
    s = R.Scene(sd0, device=0, updatable=True, keep_previous=True)
    cam = R.Camera.for_scene(sd0, (w, h))
    r = R.MegakernelRenderer(s, (w, h), depth, spp)
    seq = []
    for f in range(n_frames):
        if f:
            s.update(instances=spin_about_centre(sd0, 1.0 * f))
        r.set_frame_seed(f + 1)
        seq.append((r.render_frame(cam, want_u8=False).rgba_f32, s.gbuffer_motion(cam), float(s.scale())))
    ref = R.MegakernelRenderer(s, (w, h), depth, 1024).render_frame(cam, want_u8=False).rgba_f32
    grid = {}
    acc = R.TemporalAccumulator(0, w, h)
    for mh, frac, cn in itertools.product((4, 8, 16, 32, 64), (0.01, 0.05, 0.2, float("inf")), (-1.0, 0.5, 0.9, 0.99)):
        acc.reset()
        for frame, g, scale in seq:
            sig = float("inf") if np.isinf(frac) else float(np.float32(frac) * np.float32(scale))
            o, _, n = acc.accumulate(frame, g, cam, want_u8=False, max_history=mh, sigma_position=sig, cos_normal=cn)
        grid[f"max_history={mh} xfrac={frac} cos={cn}"] = dict(rmse=rmse(o, ref), mean_history=float(n.mean()))
    s.close()
    best = dict(sorted(grid.items(), key=lambda kv: kv[1]["rmse"])[:8])
    dflt = grid[f"max_history={R.TEMPORAL_MAX_HISTORY} xfrac={R.TEMPORAL_POSITION_FRACTION} cos={R.TEMPORAL_COS_NORMAL}"]
    return dict(raw=rmse(seq[-1][0], ref), defaults=dflt, best8=best, grid=grid)


def main():
    out = {"cost_atrium_1920x1080": cost()}
    print(json.dumps(out["cost_atrium_1920x1080"]), flush=True)
    out["update_snapshot"] = snapshot()
    print(json.dumps(out["update_snapshot"]), flush=True)
    out["sweep_rmse_linear_vs_1024spp_320x180"] = {}
    for name in ("atrium", "cornell"):
        sw = sweep(name)
        out["sweep_rmse_linear_vs_1024spp_320x180"][name] = sw
        print(name, json.dumps({k: sw[k] for k in ("raw", "defaults", "best8")}), flush=True)
    out["defaults"] = dict(max_history=R.TEMPORAL_MAX_HISTORY, position_fraction=R.TEMPORAL_POSITION_FRACTION, cos_normal=R.TEMPORAL_COS_NORMAL)
    dst = Path(sys.argv[1]) if len(sys.argv) > 1 else REPO / "profiles" / "temporal_probe.json"
    dst.parent.mkdir(parents=True, exist_ok=True)
    dst.write_text(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
