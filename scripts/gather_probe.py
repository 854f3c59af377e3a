"""Device time of the gather queries -> profiles/gather_probe.json.

    python scripts/gather_probe.py [profiles/gather_probe.json]

One process, hipEvents on one stream, 3 warm-up and 20 timed runs per case: median, min and max. Both legs on the detail-4 atrium, depth 10.
  (a) filled       2^20 points on triangle surfaces (random triangles, random barycentrics) with the unit face normals, 16 samples: one
                   rt_gather_paths_device call, beside one rt_trace_paths_device call over the same work expanded on the host to 2^24
                   single-sample rays (every point 16 times, direction = normal + the numpy model's unit vector on arbitrary states: equal
                   work, not equal bits). The windows alternate gather, expanded, gather: the two gather windows are the run-to-run spread
                   the difference is held against.
  (b) under-filled the 32 x 32 x 32 grid of scripts/path_query_probe.py with the six axis normals per point (196,608 entries: about half
                   the resident lanes), 64 samples.
Rates are rays traced (the sum of the `rays` output) over the median time. No pass mark: the figures are reported as they are."""
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "sycl-ray-tracer_amd"))
from rtamd import renderer as R  # noqa: E402
from rtamd import scenes  # noqa: E402

DEPTH = 10
WARM, RUNS = 3, 20
POINTS, SAMPLES_A = 1 << 20, 16
GRID, SAMPLES_B = 32, 64
f32 = np.float32


def xorshift(x):
    x = x.copy()
    x ^= x << np.uint32(13)
    x ^= x >> np.uint32(17)
    x ^= x << np.uint32(5)
    return x.astype(f32) * f32(1.0 / 4294967296.0), x


def unit_vectors(state):
    """random_unit_vector on an array of states (tests/test_gather.py: unit_vector_model)"""
    comp = []
    for _ in range(3):
        u, state = xorshift(state)
        comp.append(f32(-1.0) + f32(2.0) * u)
    x, y, z = comp
    inv = f32(1.0) / np.sqrt((x * x + y * y) + z * z)
    return np.stack([x * inv, y * inv, z * inv], 1)


def surface_points(sd, n, rng):
    """(pos, unit face normal) of n points on random world triangles, float32"""
    tris = sd.world_triangles()[rng.integers(0, sd.n_triangles, n)]
    u, v = rng.uniform(size=n), rng.uniform(size=n)
    fold = u + v > 1.0
    u, v = np.where(fold, 1.0 - u, u)[:, None], np.where(fold, 1.0 - v, v)[:, None]
    e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    face = np.cross(e1, e2)
    face /= np.linalg.norm(face, axis=1, keepdims=True)
    return (tris[:, 0] + u * e1 + v * e2).astype(f32), face.astype(f32)


def grid_points(sd):
    """the 32^3 grid of path_query_probe.py inside the bounds, every point with the six axis normals: an ambient cube per point"""
    tw = sd.world_triangles().reshape(-1, 3)
    lo, hi = tw.min(0), tw.max(0)
    g = (np.arange(GRID) + 0.5) / GRID
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) * (hi - lo) * 0.9 + lo + 0.05 * (hi - lo)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f32)
    return np.repeat(pts, 6, 0).astype(f32), np.tile(axes, (len(pts), 1))


def states(n, rng):
    return rng.integers(1, 2**32, n, dtype=np.uint64).astype(np.uint32)


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


def rate(t, rays_tensor, entries):
    import torch
    t["rays"] = int(rays_tensor.view(torch.int32).to(torch.int64).sum().item())
    t["mrays_per_s"] = t["rays"] / t["median_ms"] * 1e-3
    t["entries"] = entries
    return t


def main(dest: Path):
    import torch
    sd = scenes.get_scene("atrium")
    s = R.Scene(sd, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(7)
    result = {"scene": "atrium", "depth": DEPTH, "warmup": WARM, "runs": RUNS}

    def cuda(a):
        return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()

    # (a) a filled device: the gather beside the same work as one expanded path query
    pos, nrm = surface_points(sd, POINTS, rng)
    n, m = POINTS, POINTS * SAMPLES_A
    st = states(n, rng)
    epos, enrm = np.repeat(pos, SAMPLES_A, 0), np.repeat(nrm, SAMPLES_A, 0)
    edir = enrm + unit_vectors(states(m, rng))
    est = states(m, rng)
    d_pos, d_nrm, d_st = cuda(pos), cuda(nrm), cuda(st)
    d_epos, d_edir, d_est = cuda(epos), cuda(edir), cuda(est)
    del epos, enrm, edir
    rad, rays = torch.empty((n, 3), dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    erad, erays = torch.empty((m, 3), dtype=torch.float32, device="cuda"), torch.empty(m, dtype=torch.int32, device="cuda")

    def gather():
        s.gather_paths_device(n, d_pos.data_ptr(), d_nrm.data_ptr(), d_st.data_ptr(), rad.data_ptr(), DEPTH, samples=SAMPLES_A,
                              d_rays=rays.data_ptr(), stream=stream)

    def expanded():
        s.trace_paths_device(m, d_epos.data_ptr(), d_edir.data_ptr(), d_est.data_ptr(), erad.data_ptr(), DEPTH, d_rays=erays.data_ptr(), stream=stream)

    a_gather = rate(timed(gather), rays, n)
    a_expanded = rate(timed(expanded), erays, m)
    a_gather2 = rate(timed(gather), rays, n)  # the gather again behind the expanded call: the spread between two windows of the same code
    assert bool(torch.isfinite(rad).all()) and bool(torch.isfinite(erad).all())
    g_ns = [t["median_ms"] * 1e6 / t["rays"] for t in (a_gather, a_gather2)]
    e_ns = a_expanded["median_ms"] * 1e6 / a_expanded["rays"]
    result["filled"] = {"points": n, "samples": SAMPLES_A, "gather": a_gather, "expanded_path_query": a_expanded, "gather_again": a_gather2,
                        "ns_per_ray": {"gather": g_ns[0], "gather_again": g_ns[1], "expanded_path_query": e_ns},
                        "gather_window_spread": abs(g_ns[0] - g_ns[1]) / min(g_ns),
                        "gather_over_expanded_per_ray": min(g_ns) / e_ns}
    del d_pos, d_nrm, d_st, d_epos, d_edir, d_est, rad, rays, erad, erays

    # (b) an under-filled device: ambient cubes on a grid
    pos, nrm = grid_points(sd)
    k = len(pos)
    d_pos, d_nrm, d_st = cuda(pos), cuda(nrm), cuda(states(k, rng))
    rad, rays = torch.empty((k, 3), dtype=torch.float32, device="cuda"), torch.empty(k, dtype=torch.int32, device="cuda")

    def cubes():
        s.gather_paths_device(k, d_pos.data_ptr(), d_nrm.data_ptr(), d_st.data_ptr(), rad.data_ptr(), DEPTH, samples=SAMPLES_B,
                              d_rays=rays.data_ptr(), stream=stream)

    b = rate(timed(cubes), rays, k)
    b2 = rate(timed(cubes), rays, k)
    assert bool(torch.isfinite(rad).all())
    result["under_filled"] = {"grid": GRID, "normals_per_point": 6, "samples": SAMPLES_B, "gather": b, "gather_again": b2,
                              "gather_window_spread": abs(b["median_ms"] - b2["median_ms"]) / min(b["median_ms"], b2["median_ms"])}
    s.close()
    dest.parent.mkdir(parents=True, exist_ok=True)
    dest.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main(Path(sys.argv[1]) if len(sys.argv) > 1 else REPO / "profiles" / "gather_probe.json")
