"""Device time of a reflection-probe set's bake, of its prefilter and of its sample kernel, and what a sampled capture is worth
 -> profiles/reflection_probe_probe.json.

    python scripts/reflection_probe_probe.py [profiles/reflection_probe_probe.json] [--prefilter-only]

One process, hipEvents on one stream, 3 warm-up and 20 timed runs per window: median, min and max.
  bake       the detail-4 atrium, 16 probes on a 4 x 1 x 4 grid inside its bounds, size 64, 5 levels, 4 samples per texel, depth 10
             (1,572,864 entries). In this order: the bare rt_trace_paths_device over the bake's own entries (from
             rt_reflection_probes_entries_device), rt_reflection_probes_bake_device, the bare path query again (the two path windows are
             the run-to-run spread the bake's overhead is held against), rt_reflection_probes_entries_device alone and
             rt_reflection_probes_prefilter_device alone. k_rf_resolve is a difference of medians: bake - paths - entries - prefilter.
  prefilter  16 probes of size 64 with 5 levels and of size 128 with 6 levels, on synthetic captures: ms per probe, and the ratio to the
             bound stated in DESIGN.md §23 from the term count, 6 * size^2 * sum over l of 6 * S_l^2 terms of 18 + q_l vector operations
             at one operation per lane and clock: half the 157.3 TFLOPS vector peak, since nothing is fused.
  sample     2^22 points over the bake's 16 probes: coherent (per probe the directions of a 512 x 512 latitude-longitude image, in
             order) and the same points shuffled, with boxes and positions; ns per point.
  quality    the Cornell box, one probe at the room's centre, size 64, 16 samples per texel, depth 10: sample at lod 0 along 384 directions
             (the texel centres of a size-8 cube) against rt_trace_paths with 4,096 paths along the same directions. The capture's texel is a
             mean over its solid angle and the bilinear lookup mixes four of them; the reference is the radiance along one ray: the RMSE
             documents the difference.
--prefilter-only runs the prefilter windows alone (the comparison of builds that feed k_rf_prefilter's source another way, RT_MI355X_LIB).
No pass mark: the figures are reported as they are."""
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "sycl-ray-tracer_amd"))
from rtamd import scenes  # noqa: E402
from rtamd import renderer as R  # noqa: E402

DEPTH, SEED = 10, 7
WARM, RUNS = 3, 20
PROBES, SIZE, LEVELS, SPT = 16, 64, 5, 4
POINTS = 1 << 22
PEAK_OPS_PER_CU = 157.3e12 / 2 / 256  # unfused vector operations per second and CU: half the 157.3 TFLOPS peak (128 lanes x 2.4 GHz)
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


def probe_positions(sd):
    """16 positions on a 4 x 1 x 4 grid at mid height, a fifth of the extent inside the scene's bounds, and boxes of a grid cell each"""
    v = np.asarray(sd.world_triangles(), np.float64).reshape(-1, 3)
    lo, ext = v.min(0), v.max(0) - v.min(0)
    gx, gz = np.meshgrid(np.linspace(0.2, 0.8, 4), np.linspace(0.2, 0.8, 4), indexing="ij")
    pos = lo + np.stack([gx.reshape(-1), np.full(16, 0.5), gz.reshape(-1)], 1) * ext
    half = np.array([0.1, 0.5, 0.1]) * ext
    return pos.astype(f32), np.concatenate([pos - half, pos + half], 1).astype(f32)


def synthetic_level0(count, size, seed):
    g = np.random.default_rng(seed)
    lv = np.ones((count, 6, size, size, 4), f32)
    lv[..., :3] = g.uniform(0.1, 3.0, size=(count, 6, size, size, 3)).astype(f32)
    return lv


def prefilter_terms(size, levels):
    """(terms, vector operations) of one probe's prefilter. A term as the kernel writes it: 5 operations for the dot, 1 compare, q_l
    squarings, 1 for w, 4 adds and 3 multiplies for the sums, 4 selects: 18 + q_l"""
    terms = ops = 0
    for l in range(1, levels):
        t = 6 * size * size * 6 * (size >> l) ** 2
        terms += t
        ops += t * (18 + 2 * (levels - l) - 1)
    return terms, ops


def prefilter_case(s, size, levels, count=PROBES):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    props = torch.cuda.get_device_properties(0)
    r = R.ReflectionProbes(s, np.zeros((count, 3), f32), size, levels, 1)
    r.set_level0(synthetic_level0(count, size, size))
    t = timed(lambda: r.prefilter_device(stream=stream))
    chain = r.get_chain()
    terms, ops = prefilter_terms(size, levels)
    bound_ms = ops / (props.multi_processor_count * PEAK_OPS_PER_CU) * 1e3
    t.update(size=size, levels=levels, probes=count, ms_per_probe=t["median_ms"] / count, terms_per_probe=terms, vector_ops_per_probe=ops,
             compute_units=props.multi_processor_count, bound_ms_per_probe=bound_ms,
             measured_over_bound=t["median_ms"] / count / bound_ms, gterms_per_s=terms * count / t["median_ms"] * 1e-6,
             chain_checksum=float(chain.astype(np.float64).sum()), chain_finite=bool(np.isfinite(chain).all()))
    r.close()
    return t


def bake_case(s, sd):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    pos, boxes = probe_positions(sd)
    r = R.ReflectionProbes(s, pos, SIZE, LEVELS, SPT, boxes=boxes)
    n = PROBES * r.face0 * SPT
    org, d, rad = (torch.empty((n, 3), dtype=torch.float32, device="cuda") for _ in range(3))
    state, rays = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")

    def entries():
        r.entries_device(SPT, SEED, org.data_ptr(), d.data_ptr(), state.data_ptr(), stream=stream)

    def paths():
        s.trace_paths_device(n, org.data_ptr(), d.data_ptr(), state.data_ptr(), rad.data_ptr(), DEPTH, d_rays=rays.data_ptr(), stream=stream)

    def baked():
        r.bake_device(SPT, DEPTH, 0, SEED, d_stats=stats.data_ptr(), stream=stream)

    entries()
    p0 = timed(paths)
    b = timed(baked)
    p1 = timed(paths)
    e = timed(entries)
    f = timed(lambda: r.prefilter_device(stream=stream))
    torch.cuda.synchronize()
    w = stats.cpu().numpy()
    st = {"probes": int(w.view(np.uint32)[0]), "valid": int(w.view(np.uint32)[1]), "rays": int(w.view(np.uint64)[1])}
    paths_ms = min(p0["median_ms"], p1["median_ms"])
    out = {"probes": PROBES, "size": SIZE, "levels": LEVELS, "spt": SPT, "entries": n, "stats": st, "paths": p0, "bake": b, "paths_again": p1,
           "entries_device": e, "prefilter_device": f, "paths_window_spread_ms": abs(p0["median_ms"] - p1["median_ms"]),
           "bake_minus_paths_ms": b["median_ms"] - paths_ms, "bake_over_paths": b["median_ms"] / paths_ms,
           "derived_ms": {"entries": e["median_ms"], "prefilter": f["median_ms"],
                          "resolve": b["median_ms"] - paths_ms - e["median_ms"] - f["median_ms"]},
           "mrays_per_s_bake": st["rays"] / b["median_ms"] * 1e-3}
    return out, r


def sample_case(r, seed):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    g = np.random.default_rng(seed)
    per = POINTS // r.count
    side = int(np.sqrt(per))
    assert side * side * r.count == POINTS
    v, u = np.meshgrid((np.arange(side) + 0.5) / side, (np.arange(side) + 0.5) / side, indexing="ij")
    z = 1 - 2 * v.reshape(-1)
    rad, phi = np.sqrt(1 - z * z), 2 * np.pi * u.reshape(-1)
    d1 = np.stack([rad * np.cos(phi), z, rad * np.sin(phi)], 1).astype(f32)
    dirs = np.tile(d1, (r.count, 1))
    idx = np.repeat(np.arange(r.count), per).astype(np.uint32)
    half = (r.boxes[:, 3:] - r.boxes[:, :3]) * f32(0.4)
    pos = (r.positions[idx] + g.uniform(-1, 1, size=(POINTS, 3)).astype(f32) * half[idx]).astype(f32)
    lod = g.uniform(0, r.levels - 1, POINTS).astype(f32)
    perm = g.permutation(POINTS)
    out = {"probes": r.count, "chain_bytes": r.count * r.chain_texels * 16, "points": POINTS}
    rgb = torch.empty((POINTS, 3), dtype=torch.float32, device="cuda")
    first = None
    for name, order in (("coherent", None), ("shuffled", perm)):
        t_idx, t_pos, t_dir, t_lod = (torch.from_numpy(np.ascontiguousarray(a if order is None else a[order])).cuda()
                                      for a in (idx.view(np.int32), pos, dirs, lod))
        t = timed(lambda: r.sample_device(POINTS, t_idx.data_ptr(), t_pos.data_ptr(), t_dir.data_ptr(), t_lod.data_ptr(), rgb.data_ptr(),
                                          stream=stream))
        torch.cuda.synchronize()
        got = rgb.cpu().numpy()
        if order is None:
            first = got
        else:  # the same points in another order give the same numbers
            t["equals_coherent"] = bool(np.array_equal(got.view(np.uint32), first[order].view(np.uint32)))
        t.update(ns_per_point=t["median_ms"] * 1e6 / POINTS, finite=bool(np.isfinite(got).all()))
        out[name] = t
    return out


def quality_case():
    sd = scenes.get_scene("cornell")
    s = R.Scene(sd, device=0)
    v = np.asarray(sd.world_triangles(), np.float64).reshape(-1, 3)
    centre = (0.5 * (v.min(0) + v.max(0))).astype(f32)[None, :]
    r = R.ReflectionProbes(s, centre, 64, 1, 16)
    _, stats = r.bake(16, DEPTH, 0, SEED)
    S = 8
    f, y, x = (a.reshape(-1) for a in np.meshgrid(np.arange(6), np.arange(S), np.arange(S), indexing="ij"))
    sc, tc = ((x + 0.5) * (2.0 / S) - 1).astype(f32), ((y + 0.5) * (2.0 / S) - 1).astype(f32)
    one = np.ones_like(sc)
    rows = [(one, -tc, -sc), (-one, -tc, sc), (sc, one, tc), (sc, -one, -tc), (sc, -tc, one), (-sc, -tc, -one)]
    d = np.zeros((len(f), 3), f32)
    for k, row in enumerate(rows):
        d[f == k] = np.stack(row, 1)[f == k]
    got = r.sample(np.zeros(len(d), np.uint32), d, 0.0).astype(np.float64)
    rep, smp = 16, 256
    g = np.random.default_rng(SEED + 1)
    states = g.integers(1, 1 << 32, len(d) * rep, dtype=np.uint64).astype(np.uint32)
    ref = s.trace_paths(np.repeat(np.broadcast_to(centre, d.shape), rep, 0), np.repeat(d, rep, 0), states, DEPTH, samples=smp)["radiance"]
    ref = ref.reshape(len(d), rep, 3).astype(np.float64).mean(1)
    err = got - ref
    out = {"size": 64, "spt": 16, "directions": len(d), "reference_paths": rep * smp, "bake_stats": stats,
           "rmse": float(np.sqrt((err ** 2).mean())), "mean_reference": float(ref.mean()), "mean_capture": float(got.mean()),
           "relative_rmse": float(np.sqrt((err ** 2).mean()) / ref.mean())}
    r.close(), s.close()
    return out


def main(dest: Path, prefilter_only: bool):
    result = {"depth": DEPTH, "warmup": WARM, "runs": RUNS}
    sd = scenes.get_scene("empty" if prefilter_only else "atrium")
    s = R.Scene(sd, device=0)
    if not prefilter_only:
        result["bake_atrium"], r = bake_case(s, sd)
        result["sample_16_probes"] = sample_case(r, 11)
        r.close()
    result["prefilter_64x5"] = prefilter_case(s, 64, 5)
    result["prefilter_128x6"] = prefilter_case(s, 128, 6)
    s.close()
    if not prefilter_only:
        result["quality_cornell"] = quality_case()
    dest.parent.mkdir(parents=True, exist_ok=True)
    dest.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--prefilter-only"]
    main(Path(args[0]) if args else REPO / "profiles" / "reflection_probe_probe.json", "--prefilter-only" in sys.argv[1:])
