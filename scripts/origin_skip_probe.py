"""What does a bounce ray pay for starting ON a surface, and how much of it does the origin skip (rt_types.h: SkipRec) take back?
Host only (rt_scene_count_visits, no GPU): closest-hit walks of the PRODUCT tree for camera rays and three generations of diffuse-like bounce
rays — as they are (mode 0), with the origin advanced by 4 pad / |n . d| so that the ray has left its own slab (mode 0: the upper bound, not
exact), and with the origin skip (mode 4: exact, the hits must be those of mode 0 for every ray).
   usage: origin_skip_probe.py [detail, default 4] [width, default 320]"""
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO)); sys.path.insert(0, str(REPO / "sycl-ray-tracer_amd"))
from rtamd import abi, scenes

detail = int(sys.argv[1]) if len(sys.argv) > 1 else 4
W = int(sys.argv[2]) if len(sys.argv) > 2 else 320
H = W * 9 // 16
lib = abi.load_library()
NONE = 0xFFFFFFFF


def walk(h, org, dirs, mode, start=None):
    n = org.shape[0]
    org = np.ascontiguousarray(org, np.float32); dirs = np.ascontiguousarray(dirs, np.float32)
    v, tt = C.c_uint64(0), C.c_uint64(0)
    t = np.zeros(n, np.float32)
    tri = np.full(n, NONE, np.uint32) if start is None else np.ascontiguousarray(start, np.uint32).copy()
    abi.check(lib.rt_scene_count_visits(h, n, abi.fptr(org), abi.fptr(dirs), mode, C.byref(v), C.byref(tt), abi.fptr(t), abi.u32ptr(tri)))
    return v.value / n, tt.value / n, t, tri


def camera_rays(sd):
    cam = abi.rt_camera()
    ce = (C.c_float * 3)(*[float(v) for v in sd.camera.position]); di = (C.c_float * 3)(*[float(v) for v in sd.camera.direction])
    abi.check(lib.rt_camera_init(C.byref(cam), W, H, ce, di, float(sd.camera.focal_length)))
    p00, du, dv, c0 = (np.array(list(getattr(cam, k)), np.float32) for k in ("pixel00", "delta_u", "delta_v", "center"))
    ys, xs = np.mgrid[0:H, 0:W]
    d = p00 + xs[..., None].astype(np.float32) * du + ys[..., None].astype(np.float32) * dv - c0
    return np.broadcast_to(c0, (H * W, 3)).copy(), d.reshape(-1, 3).astype(np.float32)


def bounce(tw, org, dirs, t, tri, rng):
    """diffuse-like continuation of the rays that hit, as scripts/quantisation_probe.py makes it (fp32 origin = org + dir * t, direction through
    half storage as the kernels keep it); also the geometric normals and the triangles the rays start on"""
    hit = tri != NONE
    w = tw[tri[hit]]
    n = np.cross(w[:, 1] - w[:, 0], w[:, 2] - w[:, 0]); n /= np.linalg.norm(n, axis=1, keepdims=True) + 1e-30
    d = dirs[hit]
    n = np.where((np.sum(n * d, 1) > 0)[:, None], -n, n)
    u = rng.uniform(-1, 1, size=n.shape); u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = (org[hit] + (d * t[hit][:, None]).astype(np.float32)).astype(np.float32)
    return o, (n + u).astype(np.float16).astype(np.float32), n, tri[hit]


print(f"node visits / triangle tests per ray on the host walk of the product tree (detail {detail}, {W}x{H} camera rays + three bounce generations)")
for name, make in (("atrium (bench scene)", lambda: scenes.atrium_scene(detail)), ("atrium_rotated (same triangles)", lambda: scenes.atrium_tilted_scene(detail, coarse=False)),
                   ("atrium_tilted (two-triangle walls)", lambda: scenes.atrium_tilted_scene(detail, coarse=True)), ("voxel terrain", lambda: scenes.voxel_scene(detail))):
    sd = make(); c = sd.to_c(); h = C.c_void_p()
    t0 = time.time()
    abi.check(lib.rt_scene_create(C.byref(c), -1, abi.RT_BVH_SAH, C.byref(h)))
    t_build = time.time() - t0
    abi.check(lib.rt_scene_check_bvh(h))
    tw = sd.world_triangles()
    ext = float(max((tw.max((0, 1)) - tw.min((0, 1))).max(), np.abs(tw).max()))
    pad = 2e-5 * ext
    print(f"{name}: {tw.shape[0]} triangles, scene scale {ext:.3g}, pad {pad:.3g}, host build + table {t_build:.2f} s, table checked")
    print(f"    {'rays':>14s} | {'on the surface':>14s} | {'past own slab':>14s} {'same hit':>8s} | {'origin skip':>14s} {'same hit':>8s} | recovered (visits / tests)")
    rng = np.random.default_rng(7)
    org, dirs = camera_rays(sd)
    _, _, t, tri = walk(h, org, dirs, 0)
    for gen in (1, 2, 3):
        org, dirs, n, start = bounce(tw, org, dirs, t, tri, rng)
        v0, t0_, t, tri = walk(h, org, dirs, 0)
        adv = (4 * pad / np.maximum(np.abs(np.sum(n * dirs, 1)), 1e-6))[:, None]
        v1, t1, _, tri1 = walk(h, (org + dirs * adv).astype(np.float32), dirs, 0)
        v4, t4, tt4, tri4 = walk(h, org, dirs, 4, start)
        same4 = bool(np.array_equal(tri4, tri) and np.array_equal(tt4, t))
        rec_v = (v0 - v4) / max(v0 - v1, 1e-9); rec_t = (t0_ - t4) / max(t0_ - t1, 1e-9)
        print(f"    gen {gen} {org.shape[0]:8d} | {v0:6.2f} / {t0_:5.2f} | {v1:6.2f} / {t1:5.2f} {np.mean(tri1 == tri):8.4f} | {v4:6.2f} / {t4:5.2f} {'all' if same4 else 'DIFFER':>8s} | {100 * rec_v:5.1f} % / {100 * rec_t:5.1f} %")
        if not same4:
            print(f"        !! {int(np.sum(tri4 != tri))} rays with another triangle, {int(np.sum(tt4 != t))} with another t")
    lib.rt_scene_destroy(h)
