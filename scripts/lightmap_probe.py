"""Device time of a lightmap bake and of its kernels -> profiles/lightmap_probe.json.

    python scripts/lightmap_probe.py [profiles/lightmap_probe.json]

One process, hipEvents on one stream, 3 warm-up and 20 timed runs per window: median, min and max. 16 samples, depth 10, one repeat.
Two atlases, because rtamd.bake.triangle_grid_uvs cannot lay the detail-4 atrium's 283,084 triangles on 1024 x 1024 (cells of 1 texel):
  atrium_4096   the detail-4 atrium on 4096 x 4096, cells of 7 texels with a gutter of 1: the smallest power-of-two atlas the unwrap accepts
  coarse_1024   the coarse atrium (235,750 triangles) on 1024 x 1024, cells of 2 texels without a gutter
Per atlas, in this order: the bare rt_gather_paths_device over the bake's own entries (positions and normals from rt_lightmap_texels_device,
the states of rtamd.bake.corner_seeds), rt_lightmap_bake_device without dilation, the bare gather again (the two gather windows are the
run-to-run spread the bake's overhead is held against), rt_lightmap_texels_device (the owner plane's fill, k_lm_owner and k_lm_texels),
and the bake with 8 dilation passes. The kernels the interface does not start alone are differences of medians: k_lm_resolve<false> = bake -
texels - gather (the bake's k_lm_texels also writes the states), one k_lm_dilate pass = (bake with 8 passes - bake) / 8.
k_lm_owner alone: one triangle over an 8192 x 8192 atlas, rt_lightmap_texels_device beside the same call on a triangle without area (the
fill and k_lm_texels over empty texels, k_lm_owner returning at once); the difference is the covering triangle's k_lm_owner and the
guides k_lm_texels computes for 2^26 covered texels, so the second figure, a triangle that covers nothing but has the whole atlas as its
box (every lane strides, no lane writes), separates the two.
No pass mark: the figures are reported as they are."""
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "sycl-ray-tracer_amd"))
from rtamd import bake, scenes  # noqa: E402
from rtamd import renderer as R  # noqa: E402

DEPTH, SAMPLES, SEED = 10, 16, 7
WARM, RUNS = 3, 20
DILATE = 8
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


def atlas_case(sd, size, gutter):
    import torch
    s = R.Scene(sd, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    n = size * size
    lm = R.Lightmap(s, bake.triangle_grid_uvs(sd.n_triangles, size, size, gutter), size, size)
    pos, nrm = (torch.empty((n, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    tri = torch.empty(n, dtype=torch.int32, device="cuda")
    state = torch.from_numpy(bake.corner_seeds(n, 1, SEED).reshape(-1).view(np.int32)).cuda()
    rad, rays = torch.empty((n, 3), dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    rgba = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    stats = torch.zeros(3, dtype=torch.int64, device="cuda")

    def texels():
        lm.texels_device(tri.data_ptr(), pos.data_ptr(), nrm.data_ptr(), stream=stream)

    def gather():
        s.gather_paths_device(n, pos.data_ptr(), nrm.data_ptr(), state.data_ptr(), rad.data_ptr(), DEPTH, samples=SAMPLES, d_rays=rays.data_ptr(),
                              stream=stream)

    def baked(dilate):
        return lambda: lm.bake_device(rgba.data_ptr(), SAMPLES, DEPTH, SEED, dilate=dilate, d_stats=stats.data_ptr(), stream=stream)

    texels()
    g0 = timed(gather)
    b0 = timed(baked(0))
    g1 = timed(gather)
    t = timed(texels)
    b8 = timed(baked(DILATE))
    torch.cuda.synchronize()
    w = stats.cpu().numpy()
    st = {"covered": int(w.view(np.uint32)[0]), "sampled": int(w.view(np.uint32)[1]), "filled": int(w.view(np.uint32)[2]), "rays": int(w.view(np.uint64)[2])}
    gather_ms = min(g0["median_ms"], g1["median_ms"])
    out = {"atlas": size, "gutter": gutter, "triangles": sd.n_triangles, "entries": n, "stats_with_dilation": st,
           "gather": g0, "bake": b0, "gather_again": g1, "texels_device": t, f"bake_dilate_{DILATE}": b8,
           "gather_window_spread_ms": abs(g0["median_ms"] - g1["median_ms"]),
           "bake_minus_gather_ms": b0["median_ms"] - gather_ms,
           "derived_ms": {"fill_owner_texels": t["median_ms"], "resolve": b0["median_ms"] - gather_ms - t["median_ms"],
                          "dilate_pass": (b8["median_ms"] - b0["median_ms"]) / DILATE},
           "mrays_per_s_bake": st["rays"] / b0["median_ms"] * 1e-3}
    lm.close(), s.close()
    return out


def owner_case():
    """k_lm_owner on one triangle over 8192 x 8192"""
    import torch
    size = 8192
    b = scenes.SceneBuilder("one")
    mesh = b.add_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 1]] * 3, [[0, 0]] * 3, [[0, 1, 2]])
    b.add_instance(mesh, b.add_material(scenes.Material()))
    s = R.Scene(b.build(), device=0)
    stream = torch.cuda.current_stream().cuda_stream
    tri = torch.empty(size * size, dtype=torch.int32, device="cuda")
    out = {"atlas": size}
    for name, uv in (("covering", [[0, 0], [2, 0], [0, 2]]), ("no_area", [[0.25, 0.25], [0.5, 0.5], [0.75, 0.75]]),
                     ("box_without_cover", [[-1, 3], [3, -1], [3.0001, -1]])):
        lm = R.Lightmap(s, np.array([uv], f32), size, size)
        out[name] = timed(lambda: lm.texels_device(tri.data_ptr(), stream=stream))
        torch.cuda.synchronize()
        out[name]["covered"] = int((tri != -1).sum().item())
        lm.close()
    out["owner_covering_upper_bound_ms"] = out["covering"]["median_ms"] - out["no_area"]["median_ms"]
    out["owner_strides_only_ms"] = out["box_without_cover"]["median_ms"] - out["no_area"]["median_ms"]
    s.close()
    return out


def main(dest: Path):
    result = {"depth": DEPTH, "samples": SAMPLES, "repeats": 1, "warmup": WARM, "runs": RUNS,
              "atrium_4096": atlas_case(scenes.get_scene("atrium"), 4096, 1),
              "coarse_1024": atlas_case(scenes.get_scene("atrium", coarse=True), 1024, 0),
              "one_triangle_8192": owner_case()}
    dest.parent.mkdir(parents=True, exist_ok=True)
    dest.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main(Path(sys.argv[1]) if len(sys.argv) > 1 else REPO / "profiles" / "lightmap_probe.json")
