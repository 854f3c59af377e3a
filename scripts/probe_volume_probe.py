"""Device time of a probe volume's bake and of its sample kernel, and what a sampled volume is worth
-> profiles/probe_volume_probe.json.

    python scripts/probe_volume_probe.py [profiles/probe_volume_probe.json] [--sample-only]

One process, hipEvents on one stream, 3 warm-up and 20 timed runs per window: median, min and max.
  bake     the detail-4 atrium, a 16 x 8 x 16 volume fitted to its bounds, 256 directions, depth 10 (524,288 entries). In this order: the
           bare rt_trace_paths_device over the bake's own entries (from rt_probe_volume_entries_device), rt_probe_volume_bake_device, the
           bare path query again (the two path windows are the run-to-run spread the bake's overhead is held against), and
           rt_probe_volume_entries_device alone. k_pv_project is a difference of medians: bake - paths - entries.
  sample   2^22 points over two tables, the bake's 2,048 probes (295 KB) and a synthetic 128 x 64 x 128 one (1,048,576 probes, 151 MB):
           coherent (a regular grid of points, each jittered inside its cell, in x-fastest order) and the same points shuffled. ns per
           point, and bytes per second against two counts kept here: per tap (8 corners x 144 bytes per point, what the lanes ask for) and
           unique (the table once), both plus the 36 bytes a point reads and writes.
  quality  the Cornell box, a 4 x 4 x 4 volume baked with 4,096 directions at depth 10: rt_probe_volume_sample at the probe positions for the
           six axis normals against rt_gather_paths with 4,096 paths (16 entries of 256) at the same points. The two differ by design (the
           gather's lobe is the reference's cube-normalised one, the volume keeps bands 0 to 2 only): the RMSE documents the difference.
--sample-only runs the sample windows alone (the comparison of builds with another register budget for k_pv_sample, RT_MI355X_LIB).
No pass mark: the figures are reported as they are."""
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "sycl-ray-tracer_amd"))
from rtamd import bake, scenes  # noqa: E402
from rtamd import renderer as R  # noqa: E402

DEPTH, SEED = 10, 7
WARM, RUNS = 3, 20
COUNT, DIRS = (16, 8, 16), 256
LARGE = (128, 64, 128)
POINTS = 1 << 22
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


def fitted(sd, count):
    """(origin, spacing) of a count grid that spans the scene's bounds, a twentieth of the extent inside them"""
    v = np.asarray(sd.world_triangles(), np.float64).reshape(-1, 3)
    lo, ext = v.min(0), v.max(0) - v.min(0)
    return lo + 0.05 * ext, 0.9 * ext / (np.array(count) - 1)


def bake_case(s, sd):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    origin, spacing = fitted(sd, COUNT)
    v = R.ProbeVolume(s, origin, spacing, COUNT, max_dirs=DIRS)
    n = v.probes * DIRS
    pos, d, rad = (torch.empty((n, 3), dtype=torch.float32, device="cuda") for _ in range(3))
    state, rays = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")

    def entries():
        v.entries_device(DIRS, SEED, pos.data_ptr(), d.data_ptr(), state.data_ptr(), stream=stream)

    def paths():
        s.trace_paths_device(n, pos.data_ptr(), d.data_ptr(), state.data_ptr(), rad.data_ptr(), DEPTH, d_rays=rays.data_ptr(), stream=stream)

    def baked():
        v.bake_device(DIRS, DEPTH, 0, SEED, d_stats=stats.data_ptr(), stream=stream)

    entries()
    p0 = timed(paths)
    b = timed(baked)
    p1 = timed(paths)
    e = timed(entries)
    torch.cuda.synchronize()
    w = stats.cpu().numpy()
    st = {"probes": int(w.view(np.uint32)[0]), "valid": int(w.view(np.uint32)[1]), "rays": int(w.view(np.uint64)[1])}
    paths_ms = min(p0["median_ms"], p1["median_ms"])
    out = {"count": list(COUNT), "dirs": DIRS, "entries": n, "stats": st, "paths": p0, "bake": b, "paths_again": p1, "entries_device": e,
           "paths_window_spread_ms": abs(p0["median_ms"] - p1["median_ms"]), "bake_minus_paths_ms": b["median_ms"] - paths_ms,
           "bake_over_paths": b["median_ms"] / paths_ms,
           "derived_ms": {"entries": e["median_ms"], "project": b["median_ms"] - paths_ms - e["median_ms"]},
           "mrays_per_s_bake": st["rays"] / b["median_ms"] * 1e-3}
    return out, v


def grid_points(origin, spacing, count, n, seed):
    """n points on a regular grid over the volume, x fastest, each jittered inside its cell, and unit normals"""
    g = np.random.default_rng(seed)
    side = (256, 128, n // (256 * 128))
    assert side[0] * side[1] * side[2] == n
    iz, iy, ix = np.meshgrid(*(np.arange(c) for c in side[::-1]), indexing="ij")
    cell = (np.stack([ix, iy, iz], -1).reshape(-1, 3) + g.uniform(size=(n, 3))) / np.array(side)
    top = np.asarray(origin, np.float64) + np.asarray(spacing, np.float64) * (np.array(count) - 1)
    pos = (np.asarray(origin, np.float64) + cell * (top - np.asarray(origin, np.float64))).astype(f32)
    nrm = g.normal(size=(n, 3))
    return pos, (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(f32)


def sample_case(v, seed):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    pos, nrm = grid_points(v.origin, v.spacing, v.count, POINTS, seed)
    perm = np.random.default_rng(seed + 1).permutation(POINTS)
    out = {"probes": v.probes, "table_bytes": v.probes * 144, "points": POINTS}
    rgb = torch.empty((POINTS, 3), dtype=torch.float32, device="cuda")
    per_tap, unique = POINTS * (8 * 144 + 36), v.probes * 144 + POINTS * 36
    first = None
    for name, order in (("coherent", None), ("shuffled", perm)):
        p, q = (torch.from_numpy(np.ascontiguousarray(a if order is None else a[order])).cuda() for a in (pos, nrm))
        t = timed(lambda: v.sample_device(POINTS, p.data_ptr(), q.data_ptr(), rgb.data_ptr(), stream=stream))
        torch.cuda.synchronize()
        got = rgb.cpu().numpy()
        if order is None:
            first = got
        else:  # the same points in another order give the same numbers
            t["equals_coherent"] = bool(np.array_equal(got, first[order], equal_nan=True))
        t.update(ns_per_point=t["median_ms"] * 1e6 / POINTS, per_tap_gb_per_s=per_tap / t["median_ms"] * 1e-6,
                 unique_gb_per_s=unique / t["median_ms"] * 1e-6)
        out[name] = t
    return out


def synthetic_table(probes, seed):
    g = np.random.default_rng(seed)
    sh = np.zeros((probes, 9, 4), f32)
    sh[:, :, :3] = g.normal(size=(probes, 9, 3)).astype(f32) * f32(0.3)
    sh[:, 0, :3] = g.uniform(0.5, 3.0, size=(probes, 3)).astype(f32)
    sh[:, 0, 3] = 1.0
    return sh


def quality_case():
    sd = scenes.get_scene("cornell")
    s = R.Scene(sd, device=0)
    origin, count = bake.probe_grid(sd, 0.5, 0.25)
    v = R.ProbeVolume(s, origin, 0.5, count, max_dirs=4096)
    sh, stats = v.bake(4096, DEPTH, 0, SEED)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f32)
    pos, nrm = np.repeat(v.positions(), 6, 0), np.tile(axes, (v.probes, 1))
    got = v.sample(pos, nrm).astype(np.float64)
    rep, smp = 16, 256
    states = bake.corner_seeds(len(pos), rep, SEED + 1).reshape(-1)
    ref = s.gather_paths(np.repeat(pos, rep, 0), np.repeat(nrm, rep, 0), states, DEPTH, samples=smp)["radiance"]
    ref = ref.reshape(len(pos), rep, 3).astype(np.float64).mean(1)
    err = got - ref
    out = {"count": list(count), "dirs": 4096, "points": len(pos), "gather_paths": rep * smp, "bake_stats": stats,
           "rmse": float(np.sqrt((err ** 2).mean())), "mean_reference": float(ref.mean()), "mean_volume": float(got.mean()),
           "relative_rmse": float(np.sqrt((err ** 2).mean()) / ref.mean()),
           "rmse_per_normal": {"+x -x +y -y +z -z".split()[k]: float(np.sqrt((err[k::6] ** 2).mean())) for k in range(6)}}
    v.close(), s.close()
    return out


def main(dest: Path, sample_only: bool):
    result = {"depth": DEPTH, "warmup": WARM, "runs": RUNS}
    sd = scenes.get_scene("atrium")
    s = R.Scene(sd, device=0)
    if sample_only:
        v = R.ProbeVolume(s, *fitted(sd, COUNT), COUNT, max_dirs=1)
        v.set_sh(synthetic_table(v.probes, 3))
    else:
        result["bake_atrium"], v = bake_case(s, sd)
    result["sample_16x8x16"] = sample_case(v, 11)
    v.close()
    big = R.ProbeVolume(s, *fitted(sd, LARGE), LARGE, max_dirs=1)
    big.set_sh(synthetic_table(big.probes, 5))
    result["sample_128x64x128"] = sample_case(big, 13)
    big.close(), s.close()
    if not sample_only:
        result["quality_cornell"] = quality_case()
    dest.parent.mkdir(parents=True, exist_ok=True)
    dest.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--sample-only"]
    main(Path(args[0]) if args else REPO / "profiles" / "probe_volume_probe.json", "--sample-only" in sys.argv[1:])
