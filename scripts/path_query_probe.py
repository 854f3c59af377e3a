"""Device time of the path queries -> profiles/path_query_probe.json.

    python scripts/path_query_probe.py [profiles/path_query_probe.json]

One process, hipEvents on one stream, 3 warm-up and 20 timed runs per case: median, min and max.
  (a) coherent  the 1920 x 1080 atrium frame at depth 10 as a chain of 4 rt_trace_paths_device calls (samples = 1) over the camera rays of
                every pixel, beside the megakernel's 4-spp frame of the same camera in the same process. The camera rays and RNG states
                of the 4 calls are made once in an untimed pass of the same chain (the camera ray on the host in numpy, as
                tests/test_path_query.py: get_ray_model states it) and kept on the device, so the timed region is the 4 launches alone.
                The chain's frame is compared with the megakernel's bit for bit before anything is timed.
  (b) incoherent  a 32 x 32 x 32 grid of points inside the atrium's bounds with 64 uniformly random directions each (2,097,152 rays),
                samples = 1, depth 10.
Rates are rays traced (the sum of the `rays` output; the frame's ray count) over the median time."""
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "sycl-ray-tracer_amd"))
from rtamd import renderer as R  # noqa: E402
from rtamd import scenes  # noqa: E402

W, H, DEPTH, SPP = 1920, 1080, 10, 4
WARM, RUNS = 3, 20
GRID, DIRS = 32, 64
f32 = np.float32


def xorshift(x):
    x = x.copy()
    x ^= x << np.uint32(13)
    x ^= x >> np.uint32(17)
    x ^= x << np.uint32(5)
    return x.astype(f32) * f32(1.0 / 4294967296.0), x


def camera_dirs(c, x, y, state):
    """get_ray's direction before the half rounding, and the state after its two draws"""
    p00, du, dv, ce = (np.array(list(a), f32) for a in (c.pixel00, c.delta_u, c.delta_v, c.center))
    centre = (p00 + x.astype(f32)[:, None] * du) + y.astype(f32)[:, None] * dv
    u0, state = xorshift(state)
    u1, state = xorshift(state)
    sample = centre + ((f32(-0.5) + u0)[:, None] * du + (f32(-0.5) + u1)[:, None] * dv)
    return sample - ce, state


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


def main(dest: Path):
    import torch
    sd = scenes.get_scene("atrium")
    s = R.Scene(sd, device=0)
    cam = R.Camera.for_scene(sd, (W, H))
    n = W * H
    stream = torch.cuda.current_stream().cuda_stream
    result = {"scene": "atrium", "depth": DEPTH, "warmup": WARM, "runs": RUNS}

    # (a) the chain's inputs, from an untimed pass of the chain itself
    y, x = np.divmod(np.arange(n, dtype=np.int64), W)
    state = (x * ((H + 7) // 8 * 8) + y).astype(np.uint32)  # the megakernel's pixel seeds
    org = torch.from_numpy(np.tile(np.array(list(cam.c.center), f32), (n, 1))).cuda()
    dirs, states = [], []
    rad = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    st_out = torch.empty(n, dtype=torch.int32, device="cuda")
    rays = torch.empty(n, dtype=torch.int32, device="cuda")
    total = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    chain_rays = 0
    for _ in range(SPP):
        d, state = camera_dirs(cam.c, x, y, state)
        dirs.append(torch.from_numpy(d).cuda()), states.append(torch.from_numpy(state.view(np.int32)).cuda())
        s.trace_paths_device(n, org.data_ptr(), dirs[-1].data_ptr(), states[-1].data_ptr(), rad.data_ptr(), DEPTH, d_rng_out=st_out.data_ptr(),
                             d_rays=rays.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        total += rad
        chain_rays += int(rays.to(torch.int64).sum().item())
        state = st_out.cpu().numpy().view(np.uint32).copy()
    mega = R.MegakernelRenderer(s, (W, H), DEPTH, SPP)
    frame = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    fr = mega.render_frame_device(cam, d_f32=frame.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    same = bool(torch.equal(torch.sqrt(total / SPP), frame.reshape(n, 4)[:, :3])) and chain_rays == fr.rays
    assert same, "the chain of path queries is not the megakernel's frame"

    def chain():
        for k in range(SPP):
            s.trace_paths_device(n, org.data_ptr(), dirs[k].data_ptr(), states[k].data_ptr(), rad.data_ptr(), DEPTH, d_rng_out=st_out.data_ptr(),
                                 d_rays=rays.data_ptr(), stream=stream)

    a_chain = timed(chain)
    a_mega = timed(lambda: mega.render_frame_device(cam, d_f32=frame.data_ptr(), stream=stream))
    a_chain2 = timed(chain)  # the chain again behind the megakernel: the spread between two windows of the same code
    for t in (a_chain, a_mega, a_chain2):
        t["rays"] = chain_rays
        t["mrays_per_s"] = chain_rays / t["median_ms"] * 1e-3
    result["coherent"] = {"width": W, "height": H, "spp": SPP, "frame_equal": same, "path_queries": a_chain, "path_queries_again": a_chain2,
                          "megakernel": a_mega, "time_ratio_to_megakernel": a_chain["median_ms"] / a_mega["median_ms"]}
    mega.close()
    del dirs, states, total, frame

    # (b) a grid of probes with random directions
    tw = sd.world_triangles().reshape(-1, 3)
    lo, hi = tw.min(0), tw.max(0)
    g = (np.arange(GRID) + 0.5) / GRID
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) * (hi - lo) * 0.9 + lo + 0.05 * (hi - lo)
    rng = np.random.default_rng(7)
    m = GRID ** 3 * DIRS
    v = rng.normal(size=(m, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    o2 = torch.from_numpy(np.repeat(pts, DIRS, 0).astype(f32)).cuda()
    d2 = torch.from_numpy(v.astype(f32)).cuda()
    st2 = torch.from_numpy(rng.integers(1, 2**32, m, dtype=np.uint64).astype(np.uint32).view(np.int32)).cuda()
    rad2 = torch.empty((m, 3), dtype=torch.float32, device="cuda")
    rays2 = torch.empty(m, dtype=torch.int32, device="cuda")

    def probes():
        s.trace_paths_device(m, o2.data_ptr(), d2.data_ptr(), st2.data_ptr(), rad2.data_ptr(), DEPTH, d_rays=rays2.data_ptr(), stream=stream)

    b = timed(probes)
    b["rays"] = int(rays2.to(torch.int64).sum().item())
    b["mrays_per_s"] = b["rays"] / b["median_ms"] * 1e-3
    b["entries"] = m
    assert bool(torch.isfinite(rad2).all())
    result["incoherent"] = b
    s.close()
    dest.parent.mkdir(parents=True, exist_ok=True)
    dest.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main(Path(sys.argv[1]) if len(sys.argv) > 1 else REPO / "profiles" / "path_query_probe.json")
