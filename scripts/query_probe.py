"""Device time of the ray queries -> profiles/query_probe.json / .txt.

Three ray sets of 2048 x 2048 = 4,194,304 rays on the atrium and on atrium_tilted:
  primary  the unjittered camera ray of every pixel (rt_scene_gbuffer's rays); set tmax: uniform in (0, scale) per ray
  ao       cosine-hemisphere directions about the G-buffer normal at the G-buffer positions (hit pixels drawn with repetition);
           set tmax: 0.05 x scale
  mix      tests/test_gpu_parity.py's random mix (origins around the scene, a third on surfaces, a quarter of the directions short);
           set tmax: uniform in (0, scale) per ray
(scale = the largest extent of the scene's bounds.) Per set, four kernels: k_intersect_batch (rt_intersect_batch; its kernel only, not its
copies), k_query<false> (CLOSEST, no tmax), k_query<true> with tmax = +inf and with the set's tmax; 2 warm-up and 5 timed calls each.

Kernel times come from a rocprofv3 kernel trace (the dispatches in launch order, matched to the labels this script writes):
    python scripts/query_probe.py run OUT                         # under: rocprofv3 --kernel-trace --output-format csv -d OUT/kt -- ...
    python scripts/query_probe.py report OUT [profiles/query_probe.json]
`run` also records hipEvent times of the three query launches (they include the 8-byte cursor reset in front of the kernel)."""
import csv
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "sycl-ray-tracer_amd"))
from rtamd import renderer as R  # noqa: E402
from rtamd import scenes  # noqa: E402

SIDE = 2048
N = SIDE * SIDE
WARM, RUNS = 2, 5
SCENES = ("atrium", "atrium_tilted")
VARIANTS = ("k_intersect_batch", "closest", "any_inf", "any_tmax")


def unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def primary_rays(cam):
    c = cam.c
    p00, du, dv, ce = (np.array(a, np.float32) for a in (c.pixel00, c.delta_u, c.delta_v, c.center))
    y, x = np.divmod(np.arange(N, dtype=np.int64), SIDE)
    xf, yf = x.astype(np.float32)[:, None], y.astype(np.float32)[:, None]
    d = ((p00 + xf * du) + yf * dv) - ce
    return np.broadcast_to(ce, (N, 3)).copy(), d.astype(np.float32)


def ao_rays(scene, cam, rng):
    g = scene.gbuffer(cam)
    pos, nrm = g["position"].reshape(-1, 4), g["normal"].reshape(-1, 4)
    hit = np.flatnonzero(np.isfinite(pos[:, 3]))
    idx = rng.choice(hit, N)
    p, n = pos[idx, :3], nrm[idx, :3].astype(np.float64)
    a = np.where(np.abs(n[:, :1]) > 0.9, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    t = np.cross(n, a)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(n, t)
    r1, r2 = rng.random((N, 1)), rng.random((N, 1))
    phi, sr = 2 * np.pi * r1, np.sqrt(r2)
    d = t * (np.cos(phi) * sr) + b * (np.sin(phi) * sr) + n * np.sqrt(1 - r2)
    return p.astype(np.float32), unit(d)


def mix_rays(sd, rng):
    tw = sd.world_triangles()
    lo, hi = tw.reshape(-1, 3).min(0), tw.reshape(-1, 3).max(0)
    org = rng.uniform(lo - 0.1 * (hi - lo) - 0.5, hi + 0.1 * (hi - lo) + 0.5, (N, 3)).astype(np.float32)
    dirs = rng.normal(size=(N, 3)).astype(np.float32)
    dirs[: N // 4] *= 1e-2
    dirs = dirs.astype(np.float16).astype(np.float32)
    k = N // 3
    b = rng.dirichlet((1, 1, 1), k)
    org[:k] = np.einsum("ij,ijk->ik", b, tw[rng.integers(0, sd.n_triangles, k)]).astype(np.float32)
    return org, dirs


def run(out: Path):
    import torch
    out.mkdir(parents=True, exist_ok=True)
    labels, events, hits = [], {}, {}
    for name in SCENES:
        sd = scenes.get_scene(name)
        s = R.Scene(sd, device=0)
        scale = float(s.scale())
        cam = R.Camera.for_scene(sd, (SIDE, SIDE))
        rng = np.random.default_rng(1)
        sets = {"primary": primary_rays(cam) + (rng.uniform(0, scale, N).astype(np.float32),)}
        sets["ao"] = ao_rays(s, cam, rng) + (np.full(N, np.float32(0.05 * scale)),)
        sets["mix"] = mix_rays(sd, rng) + (rng.uniform(0, scale, N).astype(np.float32),)
        for set_name, (org, dirs, tmax) in sets.items():
            key = f"{name}/{set_name}"
            o, d, tm = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (org, dirs, tmax))
            t = torch.empty(N, dtype=torch.float32, device="cuda")
            u, v = torch.empty_like(t), torch.empty_like(t)
            tri = torch.empty(N, dtype=torch.int32, device="cuda")
            occ = torch.empty(N, dtype=torch.uint8, device="cuda")
            st = torch.cuda.current_stream().cuda_stream
            calls = {
                "closest": lambda: s.trace_device(N, o.data_ptr(), d.data_ptr(), d_t=t.data_ptr(), d_u=u.data_ptr(), d_v=v.data_ptr(),
                                                  d_tri=tri.data_ptr(), stream=st),
                "any_inf": lambda: s.trace_device(N, o.data_ptr(), d.data_ptr(), d_occluded=occ.data_ptr(), any_hit=True, stream=st),
                "any_tmax": lambda: s.trace_device(N, o.data_ptr(), d.data_ptr(), d_tmax=tm.data_ptr(), d_occluded=occ.data_ptr(), any_hit=True,
                                                   stream=st),
            }
            for k in range(WARM + RUNS):
                ib = s.intersect(org, dirs)
                labels.append([key, "k_intersect_batch", k >= WARM])
            hits[key] = {"closest_hits": int((ib[3] != 0xFFFFFFFF).sum())}
            for var, fn in calls.items():
                ms = []
                for k in range(WARM + RUNS):
                    torch.cuda.synchronize()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    labels.append([key, var, k >= WARM])
                    if k >= WARM:
                        ms.append(a.elapsed_time(b))
                events[f"{key}/{var}"] = float(np.median(ms))
                if var == "closest":  # the query answers as rt_intersect_batch does (tests/test_gpu_ray_query.py pins it on smaller sets)
                    assert np.array_equal(tri.cpu().numpy().view(np.uint32), ib[3]) and np.array_equal(t.cpu().numpy(), ib[0]), key
                if var == "any_tmax":
                    hits[key]["occluded_tmax"] = int(occ.sum().item())
            del o, d, tm, t, u, v, tri, occ
        s.close()
    (out / "labels.json").write_text(json.dumps({"labels": labels, "event_ms": events, "hits": hits}))
    print(f"{len(labels)} labelled launches -> {out / 'labels.json'}")


def report(out: Path, dest: Path):
    meta = json.loads((out / "labels.json").read_text())
    traces = sorted(out.rglob("*kernel_trace.csv"))
    assert traces, f"no kernel trace under {out}"
    rows = []
    for p in traces:
        with open(p) as f:
            rows += [r for r in csv.DictReader(f) if "k_intersect_batch" in r["Kernel_Name"] or "k_query" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    labels = meta["labels"]
    assert len(rows) == len(labels), f"{len(rows)} dispatches in the trace, {len(labels)} labelled"
    times = {}
    for r, (key, var, timed) in zip(rows, labels):
        want = "k_intersect_batch" if var == "k_intersect_batch" else ("k_query<true>" if var.startswith("any") else "k_query<false>")
        assert want in r["Kernel_Name"].replace(" ", ""), (want, r["Kernel_Name"])
        if timed:
            times.setdefault(key, {}).setdefault(var, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    result = {"rays_per_set": N, "runs": RUNS, "sets": {}}
    lines = [f"{'set':24s} " + " ".join(f"{v:>22s}" for v in VARIANTS), f"{'':24s} " + " ".join(f"{'ms  Grays/s':>22s}" for _ in VARIANTS)]
    for key, per in times.items():
        med = {v: float(np.median(per[v])) for v in VARIANTS}
        result["sets"][key] = {v: {"kernel_ms": med[v], "grays_per_s": N / med[v] * 1e-6, "event_ms": meta["event_ms"].get(f"{key}/{v}")}
                               for v in VARIANTS}
        result["sets"][key].update(meta["hits"][key])
        lines.append(f"{key:24s} " + " ".join(f"{med[v]:11.3f} {N / med[v] * 1e-6:10.2f}" for v in VARIANTS))
    dest.write_text(json.dumps(result, indent=1) + "\n")
    dest.with_suffix(".txt").write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(Path(sys.argv[2]))
    else:
        report(Path(sys.argv[2]), Path(sys.argv[3]) if len(sys.argv) > 3 else REPO / "profiles" / "query_probe.json")
