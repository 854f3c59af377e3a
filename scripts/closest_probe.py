"""Device time of the closest-point queries -> profiles/closest_probe.json.

    python scripts/closest_probe.py [OUT.json]

One process, hipEvents on one stream, 3 warm-up and 20 timed launches per row, reported as median (min .. max) in ms. The atrium at detail
4, 2^22 points, in three sets:
  grid      a coherent 256 x 64 x 256 grid over the bounds (x fastest)
  shuffled  the same points in random order
  surface   points 1e-3 scene scales off random surface points, along a random direction
each with no radius and with a radius of 1 % of the scene scale. Beside them a scale row — rt_trace_rays_device CLOSEST over the 2^22
unjittered primary rays of a 2048 x 2048 camera — and what the host walk (rt_scene_closest_host, use_bvh = 1: the kernel's cull rule and
child order) counts per point on the first 2^16 points of each set. The figures document; they set no pass bar."""
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "sycl-ray-tracer_amd"))
from rtamd import renderer as R  # noqa: E402
from rtamd import scenes  # noqa: E402

N = 1 << 22
WARM, RUNS = 3, 20
HOST_SAMPLE = 1 << 16
f32 = np.float32


def point_sets(sd, scale, rng):
    tw = np.asarray(sd.world_triangles(), np.float64)
    lo, hi = tw.reshape(-1, 3).min(0), tw.reshape(-1, 3).max(0)
    nx, ny, nz = 256, 64, 256
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    idx = np.stack([x, y, z], -1).reshape(-1, 3)
    grid = (lo + (idx + 0.5) / np.array([nx, ny, nz]) * (hi - lo)).astype(f32)
    assert len(grid) == N
    t = tw[rng.integers(0, len(tw), N)]
    u, v = rng.uniform(size=N), rng.uniform(size=N)
    fold = u + v > 1
    u, v = np.where(fold, 1 - u, u)[:, None], np.where(fold, 1 - v, v)[:, None]
    off = rng.normal(size=(N, 3))
    off /= np.linalg.norm(off, axis=1, keepdims=True)
    surface = (t[:, 0] + u * (t[:, 1] - t[:, 0]) + v * (t[:, 2] - t[:, 0]) + 1e-3 * scale * off).astype(f32)
    return {"grid": grid, "shuffled": np.ascontiguousarray(grid[rng.permutation(N)]), "surface": surface}


def primary_rays(cam, side):
    c = cam.c
    p00, du, dv, ce = (np.array(a, f32) for a in (c.pixel00, c.delta_u, c.delta_v, c.center))
    y, x = np.divmod(np.arange(side * side, dtype=np.int64), side)
    d = ((p00 + x.astype(f32)[:, None] * du) + y.astype(f32)[:, None] * dv) - ce
    return np.broadcast_to(ce, (side * side, 3)).copy(), d.astype(f32)


def timed(fn):
    import torch
    ms = []
    for k in range(WARM + RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k >= WARM:
            ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def main(dest: Path):
    import torch
    sd = scenes.get_scene("atrium", detail=4)
    s = R.Scene(sd, device=0)
    info = s.info()
    scale = float(s.scale())
    rng = np.random.default_rng(1)
    st = torch.cuda.current_stream().cuda_stream
    result = {"scene": "atrium detail 4", "triangles": info.n_triangles, "nodes": info.n_nodes, "points": N, "warm": WARM, "runs": RUNS,
              "host_walk_sample": HOST_SAMPLE, "rows": {}}
    radius2 = f32(0.01 * scale) * f32(0.01 * scale)
    for name, pos in point_sets(sd, scale, rng).items():
        p = torch.from_numpy(pos).cuda()
        md = torch.full((N,), float(radius2), dtype=torch.float32, device="cuda")
        d2 = torch.empty(N, dtype=torch.float32, device="cuda")
        u, v = torch.empty_like(d2), torch.empty_like(d2)
        tri = torch.empty(N, dtype=torch.int32, device="cuda")
        pt = torch.empty((N, 3), dtype=torch.float32, device="cuda")
        for what, d_md in (("no radius", 0), ("radius 1 %", md.data_ptr())):
            row = timed(lambda: s.closest_points_device(N, p.data_ptr(), d_max_dist2=d_md, d_dist2=d2.data_ptr(), d_u=u.data_ptr(), d_v=v.data_ptr(),
                                                        d_tri=tri.data_ptr(), d_point=pt.data_ptr(), stream=st))
            row["mpoints_per_s"] = N / row["median_ms"] * 1e-3
            row["answered"] = int((tri != -1).sum().item())
            host = s.closest_host(pos[:HOST_SAMPLE], np.full(HOST_SAMPLE, radius2, f32) if d_md else None, use_bvh=True)
            assert np.array_equal(tri[:HOST_SAMPLE].cpu().numpy().view(np.uint32), host["tri"]), (name, what)
            assert np.array_equal(d2[:HOST_SAMPLE].cpu().numpy().view(np.uint32), host["dist2"].view(np.uint32)), (name, what)
            row["host_node_visits_per_point"] = host["node_visits"] / HOST_SAMPLE
            row["host_tri_tests_per_point"] = host["tri_tests"] / HOST_SAMPLE
            result["rows"][f"{name}, {what}"] = row
            print(f"{name:9s} {what:11s} {row['median_ms']:8.3f} ms ({row['min_ms']:.3f} .. {row['max_ms']:.3f})  {row['mpoints_per_s']:8.1f} Mpoints/s  "
                  f"host walk {row['host_node_visits_per_point']:.1f} visits, {row['host_tri_tests_per_point']:.1f} tests per point", flush=True)
        del p, md, d2, u, v, tri, pt
    side = 2048
    org, dirs = primary_rays(R.Camera.for_scene(sd, (side, side)), side)
    o, d = torch.from_numpy(org).cuda(), torch.from_numpy(dirs).cuda()
    t = torch.empty(N, dtype=torch.float32, device="cuda")
    u, v = torch.empty_like(t), torch.empty_like(t)
    tri = torch.empty(N, dtype=torch.int32, device="cuda")
    row = timed(lambda: s.trace_device(N, o.data_ptr(), d.data_ptr(), d_t=t.data_ptr(), d_u=u.data_ptr(), d_v=v.data_ptr(), d_tri=tri.data_ptr(), stream=st))
    row["mrays_per_s"] = N / row["median_ms"] * 1e-3
    result["rows"]["scale: rt_trace_rays_device CLOSEST, 2^22 primary rays"] = row
    print(f"ray query CLOSEST     {row['median_ms']:8.3f} ms ({row['min_ms']:.3f} .. {row['max_ms']:.3f})  {row['mrays_per_s']:8.1f} Mrays/s", flush=True)
    s.close()
    dest.parent.mkdir(parents=True, exist_ok=True)
    dest.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main(Path(sys.argv[1]) if len(sys.argv) > 1 else REPO / "profiles" / "closest_probe.json")
