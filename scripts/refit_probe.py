"""Dynamic scenes on the GPU box: what rt_scene_update costs against building the scene again, and what a refit costs in tree quality.

On the atrium (detail 4, the bench scene) at 1920x1080 and 64 spp, one process:
  - rt_scene_update device_ms (hipEvents around the update's device work) and wall time: transforms only (every instance turned about the
    vertical axis through the scene's centre), and positions + normals; warm-up updates first, then the median and spread of the timed ones;
  - rt_scene_create wall time with each builder (SAH and LBVH on the host, LBVH_GPU on the device), the median of a few;
  - sah_cost and the frame time (device_ms, median of 3 after a warm-up frame) of the built scene, of the refit scene turned by DEG, and of
    a fresh SAH build of the turned scene (the same image: the frame is independent of the tree).
Usage: python scripts/refit_probe.py [DEG] [RENDERER] [updates] > out.txt   (DEG 30 by default, RENDERER wavefront | megakernel; "updates":
the update and creation times only, no frames — what an A/B of two libraries, RT_MI355X_LIB, repeats run by run)"""
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO)); sys.path.insert(0, str(REPO / "sycl-ray-tracer_amd"))
import numpy as np  # noqa: E402
from rtamd import abi, scenes  # noqa: E402
from rtamd.renderer import Camera, MegakernelRenderer, Scene, WavefrontRenderer  # noqa: E402

sys.path.insert(0, str(REPO / "tests"))
from test_scene_update import spin_about_centre  # noqa: E402

DEG = float(sys.argv[1]) if len(sys.argv) > 1 else 30.0
CLS = MegakernelRenderer if len(sys.argv) > 2 and sys.argv[2].startswith("mega") else WavefrontRenderer
W, H, SPP, DEPTH = 1920, 1080, 64, 10


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), n=len(v))


def frame_ms(scene, cam):
    r = CLS(scene, (W, H), DEPTH, SPP)
    r.render_frame(cam, want_f32=False, want_u8=False)
    t = [r.render_frame(cam, want_f32=False, want_u8=False).device_ms for _ in range(3)]
    r.close()
    return spread(t)


def main():
    sd = scenes.atrium_scene(4)
    cam = Camera.for_scene(sd, (W, H))
    out = dict(scene="atrium detail 4", triangles=sd.n_triangles, instances=int(sd.transforms.shape[0]), renderer=CLS.__name__,
               size=f"{W}x{H}", spp=SPP, deg=DEG)

    builds = {}
    for name, bvh in (("sah", abi.RT_BVH_SAH), ("lbvh", abi.RT_BVH_LBVH), ("lbvh_gpu", abi.RT_BVH_LBVH_GPU)):
        Scene(sd, 0, bvh).close()  # (warm-up: code objects, allocator)
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            s = Scene(sd, 0, bvh)
            t.append((time.perf_counter() - t0) * 1e3)
            s.close()
        builds[name] = spread(t)
    out["create_wall_ms"] = builds

    s = Scene(sd, 0, abi.RT_BVH_SAH, updatable=True)
    info0 = s.info()
    out["device_bytes"] = dict(plain=Scene(sd, 0, abi.RT_BVH_SAH).info().device_bytes, updatable=info0.device_bytes)
    out["nodes"] = info0.n_nodes
    angles = [DEG * (k % 7 + 1) / 7.0 for k in range(20)]
    centre = (np.array(info0.bounds_lo, np.float64) + np.array(info0.bounds_hi, np.float64)) / 2
    poses = [spin_about_centre(sd, a, centre=centre) for a in angles]
    for p in poses[:3]:
        s.update(instances=p)
    dev, wall = [], []
    for p in poses[3:]:
        t0 = time.perf_counter()
        st = s.update(instances=p)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(st.device_ms)
    out["update_transforms"] = dict(device_ms=spread(dev), wall_ms=spread(wall), launches=st.launches, refit_nodes=st.refit_nodes)
    rng = np.random.default_rng(1)
    verts = [(sd.positions + rng.normal(scale=1e-3, size=sd.positions.shape).astype(np.float32), sd.normals) for _ in range(12)]
    for p, n in verts[:2]:
        s.update(positions=p, normals=n)
    dev, wall = [], []
    for p, n in verts[2:]:
        t0 = time.perf_counter()
        st = s.update(positions=p, normals=n)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(st.device_ms)
    out["update_positions_normals"] = dict(device_ms=spread(dev), wall_ms=spread(wall), launches=st.launches)
    s.close()
    if "updates" in sys.argv[3:]:
        print(json.dumps(out))
        return

    # tree quality: the built scene, the refit scene turned by DEG, a fresh build of the turned scene
    s = Scene(sd, 0, abi.RT_BVH_SAH, updatable=True)
    out["built"] = dict(sah_cost=s.info().sah_cost, frame_ms=frame_ms(s, cam))
    turned = spin_about_centre(sd, DEG, centre=centre)
    s.update(instances=turned)
    out["refit"] = dict(sah_cost=s.info().sah_cost, frame_ms=frame_ms(s, cam))
    fresh = Scene(s.desc, 0, abi.RT_BVH_SAH)
    out["rebuilt"] = dict(sah_cost=fresh.info().sah_cost, frame_ms=frame_ms(fresh, cam))
    fresh.close()
    s.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
