"""Device time of the occlusion gathers -> profiles/occlusion_probe.json.

    python scripts/occlusion_probe.py [OUT.json]

One process, hipEvents on one stream, 3 warm-up and 20 timed launches per row, reported as median (min .. max) in ms. The atrium and the
tilted atrium at detail 4; 2^20 entries at the positions and normals of a 1024 x 1024 G-buffer (a pixel that sees the sky takes the entry of
the last pixel before it that does not), coherent (pixel order) and shuffled; samples = 1, 4 and 16; max_dist = 0.05 x the scene scale
(§14's AO set) and +inf (NULL). Beside every row the baseline a caller had before: k_query<true> through rt_trace_rays_device on exactly
the same n x samples rays, generated here with the numpy model in entry-major order and uploaded before the clock starts (28 bytes in and
one byte out per ray; the reduction to a count per entry is not timed). The probe checks that the baseline's bytes reduce to the gather's
`clear`, and records what the host walk (rt_scene_occlusion_host, use_bvh = 1) counts per ray on the first 2^14 entries. The figures
document; they set no pass bar."""
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "sycl-ray-tracer_amd"))
sys.path.insert(0, str(REPO / "scripts"))
from rtamd import renderer as R  # noqa: E402
from rtamd import scenes  # noqa: E402
from closest_probe import RUNS, WARM, timed  # noqa: E402

SIDE = 1024
N = SIDE * SIDE
SAMPLES = (1, 4, 16)
HOST_SAMPLE = 1 << 14
f32 = np.float32


def xorshift(x):
    x = x ^ (x << np.uint32(13))
    x = x ^ (x >> np.uint32(17))
    x = x ^ (x << np.uint32(5))
    return x.astype(f32) * f32(1.0 / 4294967296.0), x


def lobe_rays(nrm, state, samples):
    """the contract's directions in numpy fp32 (include/rt_mi355x.h: rt_occlusion_query): (n, samples, 3) float32 and which of them exist"""
    w, ok = np.zeros((len(nrm), samples, 3), f32), np.zeros((len(nrm), samples), bool)
    for s in range(samples):
        c = []
        for _ in range(3):
            u, state = xorshift(state)
            c.append(f32(-1.0) + f32(2.0) * u)
        x, y, z = c
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            inv = f32(1.0) / np.sqrt((x * x + y * y) + z * z)
            d = nrm + np.stack([x * inv, y * inv, z * inv], 1)
            l2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            w[:, s] = d * (f32(1.0) / np.sqrt(l2))[:, None]
        ok[:, s] = (l2 > 0) & np.isfinite(l2)
    return w, ok


def gbuffer_entries(s, sd):
    g = s.gbuffer(R.Camera.for_scene(sd, (SIDE, SIDE)))
    pos, nrm = g["position"].reshape(-1, 4), g["normal"].reshape(-1, 4)
    hit = np.isfinite(pos[:, 3]) & np.isfinite(pos[:, :3]).all(1) & np.isfinite(nrm[:, :3]).all(1) & (nrm[:, :3] != 0).any(1)
    src = np.maximum.accumulate(np.where(hit, np.arange(N), -1))
    src = np.where(src < 0, np.flatnonzero(hit)[0], src)
    return np.ascontiguousarray(pos[src, :3], f32), np.ascontiguousarray(nrm[src, :3], f32), float(hit.mean())


def main(dest: Path):
    import torch
    st = torch.cuda.current_stream().cuda_stream
    result = {"entries": N, "warm": WARM, "runs": RUNS, "host_walk_sample": HOST_SAMPLE, "scenes": {}, "rows": {}}
    rng = np.random.default_rng(1)
    for scene_name, sd in (("atrium", scenes.get_scene("atrium", detail=4)), ("tilted atrium", scenes.atrium_tilted_scene(4))):
        s = R.Scene(sd, device=0)
        info, scale = s.info(), float(s.scale())
        pos0, nrm0, covered = gbuffer_entries(s, sd)
        result["scenes"][scene_name] = {"triangles": info.n_triangles, "nodes": info.n_nodes, "scale": scale, "pixels_with_a_hit": covered}
        state0 = rng.integers(1, 2**32, N, dtype=np.uint64).astype(np.uint32)
        perm = rng.permutation(N)
        for order, idx in (("coherent", np.arange(N)), ("shuffled", perm)):
            pos, nrm, state = np.ascontiguousarray(pos0[idx]), np.ascontiguousarray(nrm0[idx]), np.ascontiguousarray(state0[idx])
            p, nr = torch.from_numpy(pos).cuda(), torch.from_numpy(nrm).cuda()
            sti = torch.from_numpy(state.view(np.int32)).cuda()
            vis, bent = torch.empty(N, dtype=torch.float32, device="cuda"), torch.empty((N, 3), dtype=torch.float32, device="cuda")
            clear, rays, sto = (torch.empty(N, dtype=torch.int32, device="cuda") for _ in range(3))
            for samples in SAMPLES:
                w, ok = lobe_rays(nrm, state, samples)
                assert ok.all()  # a G-buffer normal is a unit vector: no degenerate sample, so the baseline traces the same rays
                org = torch.from_numpy(np.ascontiguousarray(np.repeat(pos, samples, axis=0))).cuda()
                dirs = torch.from_numpy(w.reshape(-1, 3)).cuda()
                occ = torch.empty(N * samples, dtype=torch.uint8, device="cuda")
                for what, radius in (("max_dist 0.05 scales", f32(0.05 * scale)), ("max_dist +inf", None)):
                    md = torch.full((N,), float(radius), dtype=torch.float32, device="cuda") if radius is not None else None
                    tm = torch.full((N * samples,), float(radius), dtype=torch.float32, device="cuda") if radius is not None else None
                    row = timed(lambda: s.gather_occlusion_device(N, p.data_ptr(), nr.data_ptr(), sti.data_ptr(), samples,
                                                                  d_max_dist=md.data_ptr() if md is not None else 0, d_visibility=vis.data_ptr(),
                                                                  d_bent=bent.data_ptr(), d_clear=clear.data_ptr(), d_rays=rays.data_ptr(),
                                                                  d_rng_out=sto.data_ptr(), stream=st))
                    base = timed(lambda: s.trace_device(N * samples, org.data_ptr(), dirs.data_ptr(), d_tmax=tm.data_ptr() if tm is not None else 0,
                                                        d_occluded=occ.data_ptr(), any_hit=True, stream=st))
                    chain_clear = samples - occ.view(N, samples).to(torch.int32).sum(1)
                    assert torch.equal(chain_clear.to(torch.int32), clear), (scene_name, order, samples, what)
                    assert int(rays.min().item()) == samples == int(rays.max().item())
                    host = s.occlusion_host(pos[:HOST_SAMPLE], nrm[:HOST_SAMPLE], state[:HOST_SAMPLE], samples,
                                            None if radius is None else np.full(HOST_SAMPLE, radius, f32), use_bvh=True)
                    assert np.array_equal(host["clear"], clear[:HOST_SAMPLE].cpu().numpy().view(np.uint32)), (scene_name, order, samples, what)
                    assert np.array_equal(host["bent"], bent[:HOST_SAMPLE].cpu().numpy()), (scene_name, order, samples, what)
                    row.update({"mrays_per_s": N * samples / row["median_ms"] * 1e-3, "baseline_median_ms": base["median_ms"], "baseline_min_ms": base["min_ms"],
                                "baseline_max_ms": base["max_ms"], "over_baseline": row["median_ms"] / base["median_ms"],
                                "occluded_share": 1.0 - float(clear.sum().item()) / (N * samples),
                                "host_node_visits_per_ray": host["node_visits"] / (HOST_SAMPLE * samples),
                                "host_tri_tests_per_ray": host["tri_tests"] / (HOST_SAMPLE * samples)})
                    result["rows"][f"{scene_name}, {order}, samples = {samples}, {what}"] = row
                    print(f"{scene_name:13s} {order:8s} samples {samples:2d} {what:20s} {row['median_ms']:8.3f} ms ({row['min_ms']:.3f} .. {row['max_ms']:.3f})  "
                          f"{row['mrays_per_s']:8.1f} Mrays/s  k_query<true> {base['median_ms']:8.3f} ms ({base['min_ms']:.3f} .. {base['max_ms']:.3f})  "
                          f"x{row['over_baseline']:.2f}  occluded {row['occluded_share']:.3f}  host walk {row['host_node_visits_per_ray']:.1f} visits, "
                          f"{row['host_tri_tests_per_ray']:.1f} tests per ray", flush=True)
                    del md, tm
                del org, dirs, occ
            del p, nr, sti, vis, bent, clear, rays, sto
        s.close()
    dest.parent.mkdir(parents=True, exist_ok=True)
    dest.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main(Path(sys.argv[1]) if len(sys.argv) > 1 else REPO / "profiles" / "occlusion_probe.json")
