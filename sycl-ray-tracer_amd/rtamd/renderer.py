"""Host-side mirror of the reference's renderer plugin surface over the C ABI.

    IRenderer.render_frame(camera, scene)            src/render.hpp:11-18
    MegakernelRenderer(img_size, max_depth, spp)     src/render_megakernel.hpp:13-19
    WavefrontRenderer(img_size, max_depth, spp)      src/render_wavefront.hpp:55-61
    Camera(img_size, center, dir, focal_length)      src/camera.hpp:74-106

All rendering happens in librt_mi355x.so (HIP, gfx950). There is no CPU path here: constructing a
Scene or renderer without the built library or without a GPU raises.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import abi
from .scenes import SceneDesc


class Camera:
    """== raytracer::Camera; the constructor arithmetic runs in rt_camera_init (host C++)."""

    def __init__(self, img_size, center, direction, focal_length: float):
        self.c = abi.rt_camera()
        lib = abi.load_library()
        ce = (C.c_float * 3)(*[float(v) for v in center])
        di = (C.c_float * 3)(*[float(v) for v in direction])
        abi.check(lib.rt_camera_init(C.byref(self.c), int(img_size[0]), int(img_size[1]), ce, di, float(focal_length)))

    @classmethod
    def for_scene(cls, desc: SceneDesc, img_size):
        p = desc.camera
        return cls(img_size, p.position, p.direction, p.focal_length)


class Scene:
    """Device-resident scene: == what raytracer::Scene hands the kernels (RTCScene + GeometryData)."""

    def __init__(self, desc: SceneDesc, device: int = 0, bvh: int = abi.RT_BVH_DEFAULT, lib=None, updatable: bool = False,
                 keep_previous: bool = False):
        """`lib`: another build of the library (abi.load_developer_library()); renderers of this scene use the same one.
        `updatable`: rt_scene_create_ex with RT_SCENE_UPDATABLE, so that update() can move instances and vertices. `keep_previous`: RT_SCENE_KEEP_PREVIOUS on
        top (needs `updatable`): the scene keeps its vertices of before the last update, what gbuffer_motion() reads."""
        self.desc = desc
        self.device = device
        self._lib = lib or abi.load_library()
        self._c = desc.to_c()
        self.h = C.c_void_p()
        if updatable or keep_previous:
            flags = (abi.RT_SCENE_UPDATABLE if updatable else 0) | (abi.RT_SCENE_KEEP_PREVIOUS if keep_previous else 0)
            abi.check(self._lib.rt_scene_create_ex(C.byref(self._c), device, bvh, flags, C.byref(self.h)), self._lib)
        else:
            abi.check(self._lib.rt_scene_create(C.byref(self._c), device, bvh, C.byref(self.h)), self._lib)

    def update(self, instances=None, positions=None, normals=None) -> abi.rt_update_stats:
        """rt_scene_update: new instance matrices and / or object-space vertices, the BVH refit in place. `instances`: (transforms (I, 16),
        normal_mats (I, 9)) or None; `positions` / `normals`: (V, 3) or None. Returns the update's statistics (device_ms, launches,
        refit_nodes). self.desc is replaced by the description the scene now behaves as (SceneDesc.updated)."""
        u = abi.rt_scene_update_desc()
        keep = []
        if instances is not None:
            xf, nm = instances
            n = int(np.asarray(xf).shape[0])
            insts = (abi.rt_instance * max(n, 1))()
            words = np.frombuffer(insts, np.float32).reshape(-1, 26)
            words[:n, :16] = np.asarray(xf, np.float32).reshape(n, 16)
            words[:n, 16:25] = np.asarray(nm, np.float32).reshape(n, 9)
            words.view(np.uint32)[:n, 25] = np.asarray(self.desc.inst_material, np.uint32)[:n]
            u.n_instances, u.instances = n, insts
            keep.append(insts)
        if positions is not None or normals is not None:
            u.n_vertices = int(self.desc.positions.shape[0])
            for name, a in (("positions", positions), ("normals", normals)):
                if a is not None:
                    a = np.ascontiguousarray(a, np.float32).reshape(-1, 3)
                    u.n_vertices = a.shape[0]
                    setattr(u, name, abi.fptr(a))
                    keep.append(a)
        st = abi.rt_update_stats()
        abi.check(self._lib.rt_scene_update(self.h, C.byref(u), C.byref(st)), self._lib)
        self.desc = self.desc.updated(instances, positions, normals)
        return st

    def info(self) -> abi.rt_scene_info_t:
        out = abi.rt_scene_info_t()
        abi.check(self._lib.rt_scene_info(self.h, C.byref(out)), self._lib)
        return out

    def check_bvh(self) -> None:
        abi.check(self._lib.rt_scene_check_bvh(self.h), self._lib)

    def intersect(self, org: np.ndarray, dirs: np.ndarray):
        org = np.ascontiguousarray(org, np.float32).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = org.shape[0]
        t, u, v = (np.zeros(n, np.float32) for _ in range(3))
        tri = np.zeros(n, np.uint32)
        abi.check(self._lib.rt_intersect_batch(self.h, n, abi.fptr(org), abi.fptr(dirs), abi.fptr(t), abi.fptr(u),
                                               abi.fptr(v), abi.u32ptr(tri)), self._lib)
        return t, u, v, tri

    def trace(self, org: np.ndarray, dirs: np.ndarray, tmax=None, any_hit: bool = False):
        """rt_trace_rays on host arrays: org, dirs (n, 3); tmax (n,) or None (+inf). Closest hit: (t, u, v, tri), a miss where no hit has
        1e-4 < t <= tmax. any_hit: the occlusion bytes (n,) uint8, 1 where such a hit exists (include/rt_mi355x.h: rt_ray_query)."""
        org = np.ascontiguousarray(org, np.float32).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = org.shape[0]
        if dirs.shape[0] != n:
            raise ValueError("org and dirs must hold the same number of rays")
        q = abi.rt_ray_query(n=n, mode=abi.RT_QUERY_ANY if any_hit else abi.RT_QUERY_CLOSEST, org=org.ctypes.data, dir=dirs.ctypes.data)
        if tmax is not None:
            tmax = np.ascontiguousarray(tmax, np.float32).reshape(-1)
            if tmax.shape[0] != n:
                raise ValueError("tmax must hold one value per ray")
            q.tmax = tmax.ctypes.data
        if any_hit:
            occ = np.zeros(n, np.uint8)
            q.occluded = occ.ctypes.data
            abi.check(self._lib.rt_trace_rays(self.h, C.byref(q)), self._lib)
            return occ
        t, u, v = (np.zeros(n, np.float32) for _ in range(3))
        tri = np.zeros(n, np.uint32)
        q.t, q.u, q.v, q.tri = t.ctypes.data, u.ctypes.data, v.ctypes.data, tri.ctypes.data
        abi.check(self._lib.rt_trace_rays(self.h, C.byref(q)), self._lib)
        return t, u, v, tri

    def trace_device(self, n: int, d_org: int, d_dir: int, d_tmax: int = 0, d_t: int = 0, d_u: int = 0, d_v: int = 0, d_tri: int = 0,
                     d_occluded: int = 0, any_hit: bool = False, stream: int = 0) -> None:
        """rt_trace_rays_device on DEVICE pointers (e.g. torch .data_ptr()), enqueued on `stream`; 0 = NULL (no tmax / output not written).
        Rejected rays are marked: t = NaN, tri = abi.RT_TRI_REJECTED, occluded = 2."""
        q = abi.rt_ray_query(n=int(n), mode=abi.RT_QUERY_ANY if any_hit else abi.RT_QUERY_CLOSEST, org=d_org or None, dir=d_dir or None,
                             tmax=d_tmax or None, t=d_t or None, u=d_u or None, v=d_v or None, tri=d_tri or None,
                             occluded=d_occluded or None)
        abi.check(self._lib.rt_trace_rays_device(self.h, C.byref(q), C.c_void_p(stream or None)), self._lib)

    # ---- what the point and list queries check and allocate alike ---------------------------------------------------------------------------
    @staticmethod
    def _check_k(k, k_max):
        """k an integer 1 .. k_max (None: no upper bound)"""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1 or (k_max is not None and k > k_max):
            raise ValueError(f"k must be an integer from 1 to {k_max}" if k_max is not None else "k must be an integer, at least 1")

    @staticmethod
    def _check_limit(limit, name):
        """max_items / max_hits: an integer, at least 1, or None"""
        if limit is not None and (isinstance(limit, bool) or not isinstance(limit, (int, np.integer)) or limit < 1):
            raise ValueError(f"{name} must be an integer, at least 1, or None")

    @staticmethod
    def _check_after(after, n, first):
        """a resume key: the pair (`first` (n,) floats, after_tri (n,) integers) or None -> (float32, uint32 arrays) or (None, None)"""
        if after is None:
            return None, None
        if not isinstance(after, (tuple, list)) or len(after) != 2:
            raise ValueError(f"after must be the pair ({first}, after_tri)")
        at, atri = np.asarray(after[0]), np.asarray(after[1])
        if at.shape != (n,) or at.dtype.kind != "f" or atri.shape != (n,) or atri.dtype.kind not in "iu":
            raise ValueError(f"after must be ({first} (n,) floats, after_tri (n,) integers)")
        return np.ascontiguousarray(at, np.float32), np.ascontiguousarray(atri).astype(np.uint32)

    @staticmethod
    def _radius2(max_dist, n, numbers_only):
        """a caller's radius, one number or (n,), none negative -> (n,) float32, the radius squared in fp32 (the ABI's radius is squared, and a
        negative one would square to a positive one), or None for None. numbers_only: a dtype that is no number is refused (the list
        queries); closest_points converts whatever numpy converts."""
        if max_dist is None:
            return None
        shape = "max_dist must be one radius or hold one per point, shape (n,)"
        if numbers_only:
            md = np.asarray(max_dist)
            if md.dtype.kind not in "fiu":
                raise ValueError(shape)
            md = md.astype(np.float32)
        else:
            md = np.asarray(max_dist, np.float32)
        if md.ndim == 0:
            md = np.full(n, md, np.float32)
        if md.shape != (n,):
            raise ValueError(shape)
        if (md < 0).any():
            raise ValueError("max_dist must not be negative")
        return np.ascontiguousarray(md * md)

    @staticmethod
    def _per_point(max_dist2, n):
        """a host diagnostic's SQUARED radii, any values: (n,) float32 or None"""
        if max_dist2 is None:
            return None
        md = np.ascontiguousarray(max_dist2, np.float32).reshape(-1)
        if md.shape[0] != n:
            raise ValueError("max_dist2 must hold one value per point")
        return md

    @staticmethod
    def _point_outputs(n):
        """a closest-point query's outputs"""
        return {"dist2": np.zeros(n, np.float32), "u": np.zeros(n, np.float32), "v": np.zeros(n, np.float32), "tri": np.zeros(n, np.uint32),
                "point": np.zeros((n, 3), np.float32)}

    @staticmethod
    def _slot_outputs(n, k, first, slots=True):
        """a list query's outputs: `first` ("t" or "dist2"), "u", "v" (n, k) float32 and "tri" (n, k) uint32 (not with slots = False), "count" (n,)"""
        out = {}
        if slots:
            out = {first: np.zeros((n, k), np.float32), "u": np.zeros((n, k), np.float32), "v": np.zeros((n, k), np.float32),
                   "tri": np.zeros((n, k), np.uint32)}
        out["count"] = np.zeros(n, np.uint32)
        return out

    def _list_host(self, call, n, k, inputs, first, use_bvh, slots) -> dict:
        """the tail of nearest_host and multihit_host: the outputs (slots = False: only "count"), the call with `inputs` (arrays or None) and
        the two counters"""
        out = self._slot_outputs(n, k, first, slots)
        ptr = lambda a: None if a is None else (abi.u32ptr if a.dtype == np.uint32 else abi.fptr)(a)
        nv, nt = C.c_uint64(0), C.c_uint64(0)
        abi.check(call(self.h, n, k, *map(ptr, inputs), 1 if use_bvh else 0, *(ptr(out.get(name)) for name in (first, "u", "v", "tri", "count")),
                       C.byref(nv), C.byref(nt)), self._lib)
        out["node_visits"], out["tri_tests"] = int(nv.value), int(nt.value)
        return out

    @staticmethod
    def _page_all(n, page, limit, first, call):
        """closest_all's and trace_all's paging: call(active, key) -> a page of `page` slots for the entries `active` behind `key` (the pair
        (`first`, tri) of their last slots, None on the first page), every entry continued until it is exhausted or holds `limit` items.
        -> CSR arrays (offsets (n + 1,) int64, `first`, u, v float32, tri uint32)"""
        active, key, pages = np.arange(n), None, []
        total = np.zeros(n, np.int64)
        while len(active):
            out = call(active, key)
            cnt = out["count"].astype(np.int64)
            if limit is not None:
                cnt = np.minimum(cnt, limit - total[active])
            pages.append((active, total[active].copy(), cnt, out))
            total[active] += cnt
            more = out["count"] == page
            if limit is not None:
                more &= total[active] < limit
            key = (np.ascontiguousarray(out[first][more, page - 1]), np.ascontiguousarray(out["tri"][more, page - 1]))
            active = active[more]
        offsets = np.zeros(n + 1, np.int64)
        np.cumsum(total, out=offsets[1:])
        res = {name: np.zeros(int(offsets[-1]), np.uint32 if name == "tri" else np.float32) for name in (first, "u", "v", "tri")}
        for entries, start, cnt, out in pages:
            slot = np.arange(page)[None, :]
            take = slot < cnt[:, None]
            at = (offsets[entries] + start)[:, None] + slot
            for name, a in res.items():
                a[at[take]] = out[name][take]
        return offsets, res[first], res["u"], res["v"], res["tri"]

    def closest_points(self, pos: np.ndarray, max_dist=None) -> dict:
        """rt_closest_points on host arrays: pos (n, 3) float32; max_dist a radius (one number or (n,)), squared here in fp32, or None
        (+inf). Returns {"dist2", "u", "v": (n,) float32, "tri": (n,) uint32, "point": (n, 3) float32, "dist": sqrt(dist2)}: the nearest
        triangle within the radius, a miss (dist2 = +inf, tri = 0xFFFFFFFF, point NaN) where there is none (include/rt_mi355x.h:
        rt_point_query)."""
        pos = np.asarray(pos)
        if pos.ndim != 2 or pos.shape[1] != 3:
            raise ValueError("pos must be (n, 3)")
        n = pos.shape[0]
        pos = np.ascontiguousarray(pos, np.float32)
        md2 = self._radius2(max_dist, n, numbers_only=False)
        q = abi.rt_point_query(n=n, pos=pos.ctypes.data, max_dist2=None if md2 is None else md2.ctypes.data)
        out = self._point_outputs(n)
        for name, a in out.items():
            setattr(q, name, a.ctypes.data)
        abi.check(self._lib.rt_closest_points(self.h, C.byref(q)), self._lib)
        out["dist"] = np.sqrt(out["dist2"])
        return out

    def closest_points_device(self, n: int, d_pos: int, d_max_dist2: int = 0, d_dist2: int = 0, d_u: int = 0, d_v: int = 0, d_tri: int = 0,
                              d_point: int = 0, stream: int = 0) -> None:
        """rt_closest_points_device on DEVICE pointers (e.g. torch .data_ptr()), enqueued on `stream`; 0 = NULL (no radius / output not
        written). d_max_dist2 holds SQUARED radii. Rejected entries are marked: dist2 = NaN, tri = abi.RT_TRI_REJECTED."""
        q = abi.rt_point_query(n=int(n), pos=d_pos or None, max_dist2=d_max_dist2 or None, dist2=d_dist2 or None, u=d_u or None, v=d_v or None,
                               tri=d_tri or None, point=d_point or None)
        abi.check(self._lib.rt_closest_points_device(self.h, C.byref(q), C.c_void_p(stream or None)), self._lib)

    def closest_host(self, pos: np.ndarray, max_dist2=None, use_bvh: bool = False) -> dict:
        """rt_scene_closest_host (host diagnostic, needs no GPU): the same query by brute force (use_bvh False) or by the kernel's walk of
        the tree, counted. max_dist2 (n,) SQUARED radii or None. Returns closest_points' arrays (without "dist") and "node_visits",
        "tri_tests"."""
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        n = pos.shape[0]
        md = self._per_point(max_dist2, n)
        out = self._point_outputs(n)
        nv, nt = C.c_uint64(0), C.c_uint64(0)
        abi.check(self._lib.rt_scene_closest_host(self.h, n, abi.fptr(pos), abi.fptr(md) if md is not None else None, 1 if use_bvh else 0,
                                                  abi.fptr(out["dist2"]), abi.fptr(out["u"]), abi.fptr(out["v"]), abi.u32ptr(out["tri"]),
                                                  abi.fptr(out["point"]), C.byref(nv), C.byref(nt)), self._lib)
        out["node_visits"], out["tri_tests"] = int(nv.value), int(nt.value)
        return out

    @staticmethod
    def _nearest_args(pos, k, max_dist, after, k_max):
        """closest_points_multi's, closest_all's and nearest_host's arguments checked: pos (n, 3); k an integer 1 .. k_max (None: no upper
        bound); max_dist a radius (one number or (n,), none negative) or None; after a pair (after_dist2 (n,) floats, after_tri (n,)
        integers) or None. -> (n, pos, max_dist2 (the radius squared in fp32) or None, after_dist2, after_tri)"""
        pos = np.asarray(pos)
        if pos.ndim != 2 or pos.shape[1] != 3:
            raise ValueError("pos must be (n, 3)")
        n = pos.shape[0]
        Scene._check_k(k, k_max)
        pos = np.ascontiguousarray(pos, np.float32)
        return (n, pos, Scene._radius2(max_dist, n, numbers_only=True)) + Scene._check_after(after, n, "after_dist2")

    def closest_points_multi(self, pos: np.ndarray, k: int, max_dist=None, after=None) -> dict:
        """rt_closest_points_multi on host arrays: the k nearest counting triangles of every point in ascending (dist2, triangle index)
        order. pos (n, 3); k 1 .. abi.RT_NEAREST_MAX; max_dist a radius (one number or (n,)), squared here in fp32 as closest_points does,
        or None (+inf); after = (after_dist2 (n,), after_tri (n,)) or None: only triangles with (dist2, tri) > (after_dist2, after_tri)
        count — the key of a page's last slot continues it. Returns {"dist2", "dist" (sqrt(dist2)), "u", "v": (n, k) float32, "tri": (n, k)
        uint32, "count": (n,) uint32}; the slots past count hold dist2 = +inf, u = v = 0, tri = 0xFFFFFFFF (include/rt_mi355x.h:
        rt_nearest_query). There is no point output: bake.contact_points re-forms it from the vertices."""
        n, pos, md2, ad, atri = self._nearest_args(pos, k, max_dist, after, abi.RT_NEAREST_MAX)
        return self._nearest_call(pos, int(k), md2, (ad, atri))

    def _nearest_call(self, pos, k, md2, key) -> dict:
        """closest_points_multi behind its checks: md2 already SQUARED (closest_all pages with the radius squared once), key = (after_dist2,
        after_tri), both arrays or both None, or None"""
        n = len(pos)
        ad, atri = key or (None, None)
        out = self._slot_outputs(n, k, "dist2")
        q = abi.rt_nearest_query(n=n, k=k, pos=pos.ctypes.data, max_dist2=None if md2 is None else md2.ctypes.data,
                                 after_dist2=None if ad is None else ad.ctypes.data, after_tri=None if atri is None else atri.ctypes.data)
        for name, a in out.items():
            setattr(q, name, a.ctypes.data)
        abi.check(self._lib.rt_closest_points_multi(self.h, C.byref(q)), self._lib)
        out["dist"] = np.sqrt(out["dist2"])
        return out

    def closest_points_multi_device(self, n: int, k: int, d_pos: int, d_max_dist2: int = 0, d_after_dist2: int = 0, d_after_tri: int = 0,
                                    d_dist2: int = 0, d_u: int = 0, d_v: int = 0, d_tri: int = 0, d_count: int = 0, stream: int = 0) -> None:
        """rt_closest_points_multi_device on DEVICE pointers (e.g. torch .data_ptr()), enqueued on `stream`; 0 = NULL (no radius / no key /
        output not written). d_max_dist2 holds SQUARED radii. The outputs hold n * k entries, point-major. Rejected entries are marked:
        every slot dist2 = NaN and tri = abi.RT_TRI_REJECTED, count = 0."""
        q = abi.rt_nearest_query(n=int(n), k=int(k), pos=d_pos or None, max_dist2=d_max_dist2 or None, after_dist2=d_after_dist2 or None,
                                 after_tri=d_after_tri or None, dist2=d_dist2 or None, u=d_u or None, v=d_v or None, tri=d_tri or None,
                                 count=d_count or None)
        abi.check(self._lib.rt_closest_points_multi_device(self.h, C.byref(q), C.c_void_p(stream or None)), self._lib)

    def nearest_host(self, pos: np.ndarray, k: int, max_dist2=None, after=None, use_bvh: bool = False, slots: bool = True) -> dict:
        """rt_scene_nearest_host (host diagnostic, needs no GPU): the same query by the sorted brute force over the triangles (use_bvh
        False) or by the kernel's walk of the tree, counted. k is any integer >= 1 here; max_dist2 (n,) SQUARED radii (any value, NaN
        included: the diagnostic refuses nothing) or None. Returns closest_points_multi's arrays (without "dist") and "node_visits",
        "tri_tests"; slots = False: only "count" and the two counters (the slot arrays are not allocated: a large k)."""
        n, pos, _, ad, atri = self._nearest_args(pos, k, None, after, None)
        md = self._per_point(max_dist2, n)
        return self._list_host(self._lib.rt_scene_nearest_host, n, int(k), (pos, md, ad, atri), "dist2", use_bvh, slots)

    def closest_all(self, pos: np.ndarray, max_dist, page: int = 8, max_items: int | None = None):
        """Every triangle within max_dist of every point, in (dist2, triangle index) order: pages of `page` triangles
        (closest_points_multi), each continued with the key of its last slot for the points that filled it, until every point is
        exhausted or holds max_items triangles. Returns CSR arrays (offsets (n + 1,) int64, dist2, u, v float32, tri uint32): point i's
        triangles are [offsets[i], offsets[i + 1]). max_dist = None (no radius: every triangle of the scene, for every point) is refused
        unless max_items is given. A host-only scene (device < 0) pages through nearest_host's brute force instead: it has no device to
        ask."""
        n, pos, md2, _, _ = self._nearest_args(pos, page, max_dist, None, abi.RT_NEAREST_MAX)
        self._check_limit(max_items, "max_items")
        if max_dist is None and max_items is None:
            raise ValueError("max_dist = None lists every triangle of the scene for every point: give max_items to bound it")
        call = self._nearest_call if self.device >= 0 else self.nearest_host
        return self._page_all(n, page, max_items, "dist2", lambda a, key: call(pos[a], page, None if md2 is None else md2[a], key))

    @staticmethod
    def _multi_args(org, dirs, k, tmax, after, k_max):
        """trace_multi's and multihit_host's arguments checked: org, dirs (n, 3); k an integer 1 .. k_max (None: no upper bound); tmax (n,)
        or None; after a pair (after_t (n,) floats, after_tri (n,) integers) or None. -> (n, org, dirs, tmax, after_t, after_tri)"""
        org, dirs = np.asarray(org), np.asarray(dirs)
        if org.ndim != 2 or org.shape[1] != 3 or dirs.shape != org.shape:
            raise ValueError("org and dirs must both be (n, 3)")
        n = org.shape[0]
        Scene._check_k(k, k_max)
        org, dirs = np.ascontiguousarray(org, np.float32), np.ascontiguousarray(dirs, np.float32)
        if tmax is not None:
            tmax = np.asarray(tmax)
            if tmax.shape != (n,) or tmax.dtype.kind not in "fiu":
                raise ValueError("tmax must hold one number per ray, shape (n,)")
            tmax = np.ascontiguousarray(tmax, np.float32)
        return (n, org, dirs, tmax) + Scene._check_after(after, n, "after_t")

    def trace_multi(self, org: np.ndarray, dirs: np.ndarray, k: int, tmax=None, after=None) -> dict:
        """rt_trace_rays_multi on host arrays: the k nearest counting hits of every ray in ascending (t, triangle index) order. org, dirs
        (n, 3); k 1 .. abi.RT_MULTIHIT_MAX; tmax (n,) or None (+inf); after = (after_t (n,), after_tri (n,)) or None: only hits with
        (t, tri) > (after_t, after_tri) count — the key of a page's last slot continues it. Returns {"t", "u", "v": (n, k) float32, "tri":
        (n, k) uint32, "count": (n,) uint32}; the slots past count hold t = +inf, u = v = 0, tri = 0xFFFFFFFF (include/rt_mi355x.h:
        rt_multihit_query)."""
        n, org, dirs, tmax, at, atri = self._multi_args(org, dirs, k, tmax, after, abi.RT_MULTIHIT_MAX)
        k = int(k)
        out = self._slot_outputs(n, k, "t")
        q = abi.rt_multihit_query(n=n, k=k, org=org.ctypes.data, dir=dirs.ctypes.data, tmax=None if tmax is None else tmax.ctypes.data,
                                  after_t=None if at is None else at.ctypes.data, after_tri=None if atri is None else atri.ctypes.data)
        for name, a in out.items():
            setattr(q, name, a.ctypes.data)
        abi.check(self._lib.rt_trace_rays_multi(self.h, C.byref(q)), self._lib)
        return out

    def trace_multi_device(self, n: int, k: int, d_org: int, d_dir: int, d_tmax: int = 0, d_after_t: int = 0, d_after_tri: int = 0, d_t: int = 0,
                           d_u: int = 0, d_v: int = 0, d_tri: int = 0, d_count: int = 0, stream: int = 0) -> None:
        """rt_trace_rays_multi_device on DEVICE pointers (e.g. torch .data_ptr()), enqueued on `stream`; 0 = NULL (no tmax / no key / output
        not written). The outputs hold n * k entries, ray-major. Rejected rays are marked: every slot t = NaN and tri = abi.RT_TRI_REJECTED,
        count = 0."""
        q = abi.rt_multihit_query(n=int(n), k=int(k), org=d_org or None, dir=d_dir or None, tmax=d_tmax or None, after_t=d_after_t or None,
                                  after_tri=d_after_tri or None, t=d_t or None, u=d_u or None, v=d_v or None, tri=d_tri or None,
                                  count=d_count or None)
        abi.check(self._lib.rt_trace_rays_multi_device(self.h, C.byref(q), C.c_void_p(stream or None)), self._lib)

    def multihit_host(self, org: np.ndarray, dirs: np.ndarray, k: int, tmax=None, after=None, use_bvh: bool = False, slots: bool = True) -> dict:
        """rt_scene_multihit_host (host diagnostic, needs no GPU): the same query by brute force over the triangles (use_bvh False) or by
        the kernel's walk of the tree, counted. k is any integer >= 1 here. Returns trace_multi's arrays and "node_visits", "tri_tests";
        slots = False: only "count" and the two counters (the slot arrays are not allocated: a large k)."""
        n, org, dirs, tmax, at, atri = self._multi_args(org, dirs, k, tmax, after, None)
        return self._list_host(self._lib.rt_scene_multihit_host, n, int(k), (org, dirs, tmax, at, atri), "t", use_bvh, slots)

    def trace_all(self, org: np.ndarray, dirs: np.ndarray, tmax=None, page: int = 8, max_hits: int | None = None):
        """Every counting hit of every ray, in (t, triangle index) order: pages of `page` hits (trace_multi), each continued with the key of
        its last slot for the rays that filled it, until every ray is exhausted or holds max_hits hits. Returns CSR arrays (offsets (n + 1,)
        int64, t, u, v float32, tri uint32): ray i's hits are [offsets[i], offsets[i + 1]). A host-only scene (device < 0) pages through
        multihit_host's brute force instead: it has no device to ask.
        The contract's limit (include/rt_mi355x.h: rt_multihit_query) holds here too: on a device scene a hit on an ill-conditioned
        triangle — a sliver whose fp32 t lies more than half the boxes' padding in front of its true t — can be missing from a ray's list
        when tmax or a page's last entry lies between the two. Every hit listed is right and listed once; the brute force has no limit."""
        n, org, dirs, tmax, _, _ = self._multi_args(org, dirs, page, tmax, None, abi.RT_MULTIHIT_MAX)
        self._check_limit(max_hits, "max_hits")
        call = self.trace_multi if self.device >= 0 else self.multihit_host
        return self._page_all(n, page, max_hits, "t", lambda a, key: call(org[a], dirs[a], page, None if tmax is None else tmax[a], key))

    @staticmethod
    def _entry_args(names, what, in0, in1, rng):
        """what the path, gather and occlusion wrappers check alike: two (n, 3) inputs (`names` in the messages) and one xorshift32 state
        per ray or entry (`what`). -> (n, in0, in1 float32, rng uint32, all contiguous)"""
        in0, in1, rng = np.asarray(in0), np.asarray(in1), np.asarray(rng)
        if in0.ndim != 2 or in0.shape[1] != 3 or in1.shape != in0.shape:
            raise ValueError(f"{names[0]} and {names[1]} must both be (n, 3)")
        n = in0.shape[0]
        if rng.shape != (n,):
            raise ValueError(f"rng must hold one state per {what}, shape (n,)")
        if rng.dtype.kind not in "ui":
            raise ValueError("rng must be an integer array (xorshift32 states)")
        return n, np.ascontiguousarray(in0, np.float32), np.ascontiguousarray(in1, np.float32), np.ascontiguousarray(rng, np.uint32)

    def _paths(self, call, query, names, fields, what, in0, in1, rng, max_depth, samples, rr_start) -> dict:
        """trace_paths and gather_paths: two (n, 3) float32 inputs (`names` in the messages, `fields` of `query`) and one xorshift32 state
        per ray or entry (`what`), through the host-array entry point `call`."""
        n, in0, in1, rng = self._entry_args(names, what, in0, in1, rng)
        out = {"radiance": np.zeros((n, 3), np.float32), "rng": np.zeros(n, np.uint32), "rays": np.zeros(n, np.uint32)}
        q = query(n=n, max_depth=int(max_depth), samples=int(samples), rr_start=int(rr_start), rng=rng.ctypes.data,
                  rng_out=out["rng"].ctypes.data, radiance=out["radiance"].ctypes.data, rays=out["rays"].ctypes.data,
                  **{fields[0]: in0.ctypes.data, fields[1]: in1.ctypes.data})
        abi.check(call(self.h, C.byref(q)), self._lib)
        return out

    def trace_paths(self, org: np.ndarray, dirs: np.ndarray, rng: np.ndarray, max_depth: int, samples: int = 1, rr_start: int = 0) -> dict:
        """rt_trace_paths on host arrays: org, dirs (n, 3) float32 and rng (n,) uint32, every ray's xorshift32 state. `samples` paths of at
        most `max_depth` rays per entry, each continuing the state the one before left. Returns {"radiance": (n, 3) float32, the mean of
        the paths' linear radiance, "rng": (n,) uint32, the states after the last path, "rays": (n,) uint32, the rays traced}
        (include/rt_mi355x.h: rt_path_query)."""
        return self._paths(self._lib.rt_trace_paths, abi.rt_path_query, ("org", "dirs"), ("org", "dir"), "ray", org, dirs, rng,
                           max_depth, samples, rr_start)

    def trace_paths_device(self, n: int, d_org: int, d_dir: int, d_rng: int, d_radiance: int, max_depth: int, samples: int = 1,
                           rr_start: int = 0, d_rng_out: int = 0, d_rays: int = 0, stream: int = 0) -> None:
        """rt_trace_paths_device on DEVICE pointers (e.g. torch .data_ptr()), enqueued on `stream`; 0 = NULL (d_rng_out, d_rays: not
        written; d_rng_out may equal d_rng). Rejected rays are marked: radiance = NaN, rays = 0xFFFFFFFF, rng_out = rng."""
        q = abi.rt_path_query(n=int(n), max_depth=int(max_depth), samples=int(samples), rr_start=int(rr_start), org=d_org or None,
                              dir=d_dir or None, rng=d_rng or None, rng_out=d_rng_out or None, radiance=d_radiance or None,
                              rays=d_rays or None)
        abi.check(self._lib.rt_trace_paths_device(self.h, C.byref(q), C.c_void_p(stream or None)), self._lib)

    def gather_paths(self, pos: np.ndarray, normals: np.ndarray, rng: np.ndarray, max_depth: int, samples: int = 1, rr_start: int = 0) -> dict:
        """rt_gather_paths on host arrays: pos, normals (n, 3) float32 and rng (n,) uint32, every entry's xorshift32 state. `samples` paths
        of at most `max_depth` rays per entry, each from pos[i] along the diffuse bounce's own direction normals[i] + random_unit_vector
        drawn from the running state. Returns {"radiance": (n, 3) float32, the mean of the paths' linear radiance, "rng": (n,) uint32, the
        states after the last path, "rays": (n,) uint32, the rays traced} (include/rt_mi355x.h: rt_gather_query)."""
        return self._paths(self._lib.rt_gather_paths, abi.rt_gather_query, ("pos", "normals"), ("pos", "normal"), "entry", pos,
                           normals, rng, max_depth, samples, rr_start)

    def gather_paths_device(self, n: int, d_pos: int, d_normal: int, d_rng: int, d_radiance: int, max_depth: int, samples: int = 1,
                            rr_start: int = 0, d_rng_out: int = 0, d_rays: int = 0, stream: int = 0) -> None:
        """rt_gather_paths_device on DEVICE pointers (e.g. torch .data_ptr()), enqueued on `stream`; 0 = NULL (d_rng_out, d_rays: not
        written; d_rng_out may equal d_rng). Rejected entries are marked: radiance = NaN, rays = 0xFFFFFFFF, rng_out = rng."""
        q = abi.rt_gather_query(n=int(n), max_depth=int(max_depth), samples=int(samples), rr_start=int(rr_start), pos=d_pos or None,
                                normal=d_normal or None, rng=d_rng or None, rng_out=d_rng_out or None, radiance=d_radiance or None,
                                rays=d_rays or None)
        abi.check(self._lib.rt_gather_paths_device(self.h, C.byref(q), C.c_void_p(stream or None)), self._lib)

    @staticmethod
    def _occlusion_args(pos, normals, rng, samples, max_dist):
        """gather_occlusion's and occlusion_host's arguments checked: pos, normals (n, 3); rng (n,) integers; samples an integer; max_dist
        one number or (n,) numbers, any sign (a negative one occludes nothing), or None (+inf). -> (n, pos, normals, rng, max_dist or None)"""
        n, pos, normals, rng = Scene._entry_args(("pos", "normals"), "entry", pos, normals, rng)
        if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)):
            raise ValueError("samples must be an integer")
        if max_dist is not None:
            md = np.asarray(max_dist)
            if md.dtype.kind not in "fiu" or md.shape not in ((), (n,)):
                raise ValueError("max_dist must be one distance or hold one per entry, shape (n,)")
            max_dist = np.ascontiguousarray(np.broadcast_to(md.astype(np.float32), (n,)))
        return n, pos, normals, rng, max_dist

    @staticmethod
    def _occlusion_query(n, samples, pos, normals, rng, max_dist):
        """the query over host arrays and its outputs {"visibility", "bent", "clear", "rays", "rng"}"""
        out = {"visibility": np.zeros(n, np.float32), "bent": np.zeros((n, 3), np.float32), "clear": np.zeros(n, np.uint32),
               "rays": np.zeros(n, np.uint32), "rng": np.zeros(n, np.uint32)}
        q = abi.rt_occlusion_query(n=n, samples=int(samples), pos=pos.ctypes.data, normal=normals.ctypes.data,
                                   max_dist=None if max_dist is None else max_dist.ctypes.data, rng=rng.ctypes.data, rng_out=out["rng"].ctypes.data,
                                   visibility=out["visibility"].ctypes.data, bent=out["bent"].ctypes.data, clear=out["clear"].ctypes.data,
                                   rays=out["rays"].ctypes.data)
        return q, out

    def gather_occlusion(self, pos: np.ndarray, normals: np.ndarray, rng: np.ndarray, samples: int, max_dist=None) -> dict:
        """rt_gather_occlusion on host arrays: pos, normals (n, 3) float32 and rng (n,) uint32, every entry's xorshift32 state. `samples`
        any-hit rays per entry from pos[i] along the diffuse bounce's own direction normals[i] + random_unit_vector, normalised, no farther
        than max_dist (one distance or (n,), world units; None: +inf). Returns {"visibility": (n,) float32, the share of the samples that met
        nothing, "bent": (n, 3) float32, the sum of the unoccluded directions over samples (not normalised: bake.normalise_bent), "clear",
        "rays": (n,) uint32, "rng": (n,) uint32, the states after the last sample} (include/rt_mi355x.h: rt_occlusion_query)."""
        n, pos, normals, rng, md = self._occlusion_args(pos, normals, rng, samples, max_dist)
        q, out = self._occlusion_query(n, samples, pos, normals, rng, md)
        abi.check(self._lib.rt_gather_occlusion(self.h, C.byref(q)), self._lib)
        return out

    def gather_occlusion_device(self, n: int, d_pos: int, d_normal: int, d_rng: int, samples: int, d_max_dist: int = 0, d_visibility: int = 0,
                                d_bent: int = 0, d_clear: int = 0, d_rays: int = 0, d_rng_out: int = 0, stream: int = 0) -> None:
        """rt_gather_occlusion_device on DEVICE pointers (e.g. torch .data_ptr()), enqueued on `stream`; 0 = NULL (no max_dist / output not
        written; d_rng_out may equal d_rng). Rejected entries are marked: visibility and bent NaN, clear = rays = 0xFFFFFFFF, rng_out = rng."""
        q = abi.rt_occlusion_query(n=int(n), samples=int(samples), pos=d_pos or None, normal=d_normal or None, max_dist=d_max_dist or None,
                                   rng=d_rng or None, rng_out=d_rng_out or None, visibility=d_visibility or None, bent=d_bent or None,
                                   clear=d_clear or None, rays=d_rays or None)
        abi.check(self._lib.rt_gather_occlusion_device(self.h, C.byref(q), C.c_void_p(stream or None)), self._lib)

    def occlusion_host(self, pos: np.ndarray, normals: np.ndarray, rng: np.ndarray, samples: int, max_dist=None, use_bvh: bool = False) -> dict:
        """rt_scene_occlusion_host (host diagnostic, needs no GPU): the same gather with every sample's any-hit query by brute force over the
        triangles (use_bvh False) or by the kernel's walk of the tree, counted. Entries are not refused here. Returns gather_occlusion's
        arrays and "node_visits", "tri_tests"."""
        n, pos, normals, rng, md = self._occlusion_args(pos, normals, rng, samples, max_dist)
        q, out = self._occlusion_query(n, samples, pos, normals, rng, md)
        nv, nt = C.c_uint64(0), C.c_uint64(0)
        abi.check(self._lib.rt_scene_occlusion_host(self.h, C.byref(q), 1 if use_bvh else 0, C.byref(nv), C.byref(nt)), self._lib)
        out["node_visits"], out["tri_tests"] = int(nv.value), int(nt.value)
        return out

    def gbuffer(self, camera: Camera) -> dict:
        """rt_scene_gbuffer: the guide images of the camera's primary hits, {"albedo", "normal", "position"}, each (H, W, 4) float32
        (include/rt_mi355x.h states what a pixel holds)."""
        w, h = int(camera.c.width), int(camera.c.height)
        out = {k: np.zeros((max(h, 0), max(w, 0), 4), np.float32) for k in ("albedo", "normal", "position")}
        abi.check(self._lib.rt_scene_gbuffer(self.h, C.byref(camera.c), abi.fptr(out["albedo"]), abi.fptr(out["normal"]),
                                             abi.fptr(out["position"])), self._lib)
        return out

    def gbuffer_device(self, camera: Camera, d_albedo: int, d_normal: int, d_position: int, stream: int = 0) -> None:
        """rt_scene_gbuffer_device: the three planes into DEVICE buffers of H*W*4 floats (e.g. torch .data_ptr()), enqueued on `stream`."""
        abi.check(self._lib.rt_scene_gbuffer_device(self.h, C.byref(camera.c), C.c_void_p(d_albedo or None), C.c_void_p(d_normal or None),
                                                    C.c_void_p(d_position or None), C.c_void_p(stream or None)), self._lib)

    def gbuffer_motion(self, camera: Camera) -> dict:
        """rt_scene_gbuffer_motion: gbuffer()'s three planes plus "prev_position", where every visible surface point was before the scene's
        last update (w = 1; zeros on a miss). The scene must have been created with keep_previous."""
        w, h = int(camera.c.width), int(camera.c.height)
        out = {k: np.zeros((max(h, 0), max(w, 0), 4), np.float32) for k in ("albedo", "normal", "position", "prev_position")}
        abi.check(self._lib.rt_scene_gbuffer_motion(self.h, C.byref(camera.c), abi.fptr(out["albedo"]), abi.fptr(out["normal"]),
                                                    abi.fptr(out["position"]), abi.fptr(out["prev_position"])), self._lib)
        return out

    def gbuffer_motion_device(self, camera: Camera, d_albedo: int, d_normal: int, d_position: int, d_prev_position: int, stream: int = 0) -> None:
        """rt_scene_gbuffer_motion_device: the four planes into DEVICE buffers of H*W*4 floats, enqueued on `stream`."""
        v = [C.c_void_p(x or None) for x in (d_albedo, d_normal, d_position, d_prev_position, stream)]
        abi.check(self._lib.rt_scene_gbuffer_motion_device(self.h, C.byref(camera.c), *v), self._lib)

    def scale(self) -> np.float32:
        """The largest extent of the scene's bounds (rt_scene_info), fp32: what the denoiser's default sigma_position is a fraction of."""
        i = self.info()
        return np.float32(max(np.float32(i.bounds_hi[a]) - np.float32(i.bounds_lo[a]) for a in range(3)))

    def scatter(self, material: int, dirs, normals, uvs, seeds):
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        uvs = np.ascontiguousarray(uvs, np.float32).reshape(-1, 2)
        seeds = np.ascontiguousarray(seeds, np.uint32)
        n = dirs.shape[0]
        ok = np.zeros(n, np.uint8)
        od, oa = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        so = np.zeros(n, np.uint32)
        abi.check(self._lib.rt_probe_scatter(self.h, material, n, abi.fptr(dirs), abi.fptr(normals), abi.fptr(uvs),
                                             abi.u32ptr(seeds), abi.u8ptr(ok), abi.fptr(od), abi.fptr(oa), abi.u32ptr(so)), self._lib)
        return ok, od, oa, so

    def shading_tables(self) -> dict:
        """rt_dev_scene_tables, for a scene built by the DEVELOPER library (Scene(..., lib=abi.load_developer_library())): whether the
        shading word is packed, the normal matrices and materials the shading kernels stage in LDS (0 in a host-only scene), the device's
        instance table as (n_rows, 9) float32 rows and every triangle's shading word (ShadeRec::instance) in scene order."""
        if not hasattr(self._lib, "rt_dev_scene_tables"):
            raise RuntimeError("shading_tables() needs a scene of the developer library")
        packed, lds_nm, lds_mats, n_rows = (C.c_uint32() for _ in range(4))
        args = (C.byref(packed), C.byref(lds_nm), C.byref(lds_mats), C.byref(n_rows))
        abi.check(self._lib.rt_dev_scene_tables(self.h, *args, None, 0, None), self._lib)
        rows = np.zeros((n_rows.value, 9), np.float32)
        words = np.zeros(self.desc.n_triangles, np.uint32)
        abi.check(self._lib.rt_dev_scene_tables(self.h, *args, abi.fptr(rows), n_rows.value, abi.u32ptr(words)), self._lib)
        return dict(packed_mat=packed.value, lds_nm=lds_nm.value, lds_mats=lds_mats.value, rows=rows, words=words)

    def tree(self) -> dict:
        """rt_dev_scene_tree, for a scene built by the DEVELOPER library: the BVH as built. `nodes` is the host copy of the node array as
        (n_nodes, 16) uint32 words (64-byte BvhNode records, child words are node indices), `global_index` every leaf-order triangle's
        scene index, `wverts` the fp32 world-space vertices the builder used as (n_triangles, 3, 3), `pad` and `bounds_lo/hi` its box
        padding and scene bounds, `stack_need` the tree's worst-case traversal stack need and `built_by` the builder that produced it
        (abi.RT_BVH_LBVH_GPU on the device, abi.RT_BVH_MEDIAN_INTERNAL after a fallback to the balanced host build)."""
        if not hasattr(self._lib, "rt_dev_scene_tree"):
            raise RuntimeError("tree() needs a scene of the developer library")
        n_nodes, n_tris, n_wverts, stack_need = (C.c_uint32() for _ in range(4))
        built_by, pad, bounds = C.c_int32(), C.c_float(), (C.c_float * 6)()
        args = (C.byref(n_nodes), C.byref(n_tris), C.byref(n_wverts), C.byref(stack_need), C.byref(built_by), C.byref(pad), bounds)
        abi.check(self._lib.rt_dev_scene_tree(self.h, *args, None, None, None, 0), self._lib)
        cap = max(n_nodes.value, n_tris.value, n_wverts.value)
        nodes = np.zeros((cap, 16), np.uint32)
        gidx = np.zeros(cap, np.uint32)
        wv = np.zeros(cap, np.float32)
        abi.check(self._lib.rt_dev_scene_tree(self.h, *args, nodes.ctypes.data_as(C.c_void_p), abi.u32ptr(gidx), abi.fptr(wv), cap), self._lib)
        b = np.frombuffer(bounds, np.float32).copy()
        return dict(nodes=nodes[: n_nodes.value], global_index=gidx[: n_tris.value], wverts=wv[: n_wverts.value].reshape(-1, 3, 3),
                    pad=np.float32(pad.value), bounds_lo=b[:3], bounds_hi=b[3:], stack_need=stack_need.value, built_by=built_by.value)

    def close(self):
        if self.h:
            self._lib.rt_scene_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class Frame:
    rgba_f32: np.ndarray | None  # (rows, W, 4) float32: sqrt(mean rgb), alpha 1 — pre-quantisation
    rgba_u8: np.ndarray | None   # (rows, W, 4) uint8: the reference's RGBA-unorm8 image
    rays: int
    seconds: float
    device_ms: float
    hot_kernel_ms: float
    hot_kernel_launches: int
    launches: int
    kernels: dict = None         # launches of the frame per kernel family (abi.KERNELS): what actually ran
    stream_lanes: int = 0        # the schedule as the library resolved it for this tile
    samples_per_launch: int = 0
    finish_depth: int = 0
    cost_ordered: bool = False
    kernel_ms: dict = None       # with profiling: summed launch durations per kernel family (hipEvents on the launches' own streams)
    hw_queues: int = 0           # GPU_MAX_HW_QUEUES as the library read it (4 = HIP's default): bounds the automatic stream lanes
    pixel_slices: int = 0        # slices a pixel's samples were rendered in (1 = every pixel on one lane, an empty tile, an unsliced schedule)

    @classmethod
    def from_stats(cls, f, b, st):
        return cls(f, b, int(st.rays), st.seconds, st.device_ms, st.hot_kernel_ms, int(st.hot_kernel_launches), int(st.launches),
                   {name: int(st.launches_by_kernel[i]) for name, i in abi.KERNELS.items()}, int(st.stream_lanes),
                   int(st.samples_per_launch), int(st.finish_depth), bool(st.cost_ordered),
                   {name: float(st.kernel_ms[i]) for name, i in abi.KERNELS.items()}, int(st.hw_queues), int(st.pixel_slices))

    def stat_lines(self) -> list[str]:
        """The three lines benchmark.py scrapes (src/render_wavefront.cpp:425-427, benchmark.py:49-55)."""
        secs = self.device_ms * 1e-3
        return [f"Time measured: {secs:.6f} seconds", f"Total rays: {self.rays}",
                f"Rays/sec: {self.rays / secs / 1e6:.2f}M"]


class IRenderer:
    """== raytracer::IRenderer (src/render.hpp:11-18)."""
    KIND = -1

    def __init__(self, scene: Scene, img_size, max_depth: int = 10, sample_count: int = 32,
                 seed_mode: int = abi.RT_SEED_DEFAULT):
        self.scene = scene
        self.img_size = (int(img_size[0]), int(img_size[1]))
        self.max_depth, self.sample_count = int(max_depth), int(sample_count)
        self._lib = scene._lib
        self.h = C.c_void_p()
        abi.check(self._lib.rt_renderer_create(self.KIND, scene.h, self.img_size[0], self.img_size[1], self.max_depth,
                                               self.sample_count, seed_mode, C.byref(self.h)), self._lib)

    def set_tile(self, rank: int, world: int, strip_rows: int = 8) -> None:
        abi.check(self._lib.rt_renderer_set_tile(self.h, rank, world, strip_rows), self._lib)

    def set_profiling(self, enable: bool) -> None:
        abi.check(self._lib.rt_renderer_set_profiling(self.h, int(enable)), self._lib)

    def set_russian_roulette(self, start_bounce: int) -> None:
        """Extension (a to-do upstream: PLAN.md:23-27): paths are thinned from bounce `start_bounce` on; 0 = off (default)."""
        abi.check(self._lib.rt_renderer_set_russian_roulette(self.h, int(start_bounce)), self._lib)

    def set_frame_seed(self, salt: int) -> None:
        """rt_renderer_set_frame_seed: the frames begun from now on start every pixel's chain at pixel_seed + salt * 0x9E3779B9 (0: the
        reference's seeds). An animation passes its frame number, so that its frames' noise is independent."""
        abi.check(self._lib.rt_renderer_set_frame_seed(self.h, int(salt) & 0xFFFFFFFF), self._lib)

    def set_schedule(self, finish_depth: int = 0, samples_per_launch: int = 0, stream_lanes: int = 0, requeue: int = -1,
                     reorder: bool = False, matsort: bool = False, cost_order: int = -1, hip_graph: bool = False,
                     fused_bounce: bool = False, pixel_slices: int = -1) -> None:
        """rt_renderer_set_schedule: which of the wavefront renderer's schedules renders the frame (same frame bit for bit; the
        reference has one: a launch per bounce, src/render_wavefront.cpp:396-417 = finish_depth=abi.RT_SCHED_ALL_BOUNCES).
        Frame.kernels reports what ran. pixel_slices (-1 automatic, 0 / 1 off, 2 .. 8: rt_mi355x.h) is the only field the megakernel uses;
        the wavefront renderer slices its one-launch schedule (samples_per_launch 0, finish_depth 0) and not with hip_graph, more than
        one stream lane or cost_order=1. Frame.pixel_slices reports what ran."""
        sc = abi.rt_schedule(int(finish_depth), int(samples_per_launch), int(stream_lanes), int(requeue), int(bool(reorder)),
                             int(bool(matsort)), int(cost_order), int(bool(hip_graph)), int(bool(fused_bounce)), int(pixel_slices))
        abi.check(self._lib.rt_renderer_set_schedule(self.h, C.byref(sc)), self._lib)

    def get_schedule(self) -> abi.rt_schedule:
        sc = abi.rt_schedule()
        abi.check(self._lib.rt_renderer_get_schedule(self.h, C.byref(sc)), self._lib)
        return sc

    @property
    def local_rows(self) -> int:
        return int(self._lib.rt_renderer_local_rows(self.h))

    def global_rows(self) -> np.ndarray:
        return np.array([self._lib.rt_renderer_global_row(self.h, i) for i in range(self.local_rows)], np.int64)

    def render_frame(self, camera: Camera, scene: Scene | None = None, want_f32: bool = True, want_u8: bool = True) -> Frame:
        if scene is not None and scene is not self.scene:
            raise ValueError("renderer was created for a different scene")
        rows, w = self.local_rows, self.img_size[0]
        f = np.zeros((rows, w, 4), np.float32) if want_f32 else None
        b = np.zeros((rows, w, 4), np.uint8) if want_u8 else None
        st = abi.rt_stats()
        abi.check(self._lib.rt_render_frame(self.h, C.byref(camera.c), abi.fptr(f) if want_f32 else None,
                                            abi.u8ptr(b) if want_u8 else None, C.byref(st)), self._lib)
        return Frame.from_stats(f, b, st)

    def render_frame_device(self, camera: Camera, d_f32: int = 0, d_u8: int = 0, stream: int = 0) -> Frame:
        """Outputs go to DEVICE pointers (e.g. torch tensor .data_ptr()); nothing is copied to host."""
        st = abi.rt_stats()
        abi.check(self._lib.rt_render_frame_device(self.h, C.byref(camera.c), C.c_void_p(d_f32 or None),
                                                   C.c_void_p(d_u8 or None), C.c_void_p(stream or None), C.byref(st)), self._lib)
        return Frame.from_stats(None, None, st)

    def begin_frame(self, camera: Camera, d_f32: int = 0, d_u8: int = 0, stream: int = 0) -> None:
        """Enqueues the frame and returns at once; collect it with end_frame(). Frames of different renderers overlap on
        the device (the next frame's waves move in while this one's last pixels drain)."""
        abi.check(self._lib.rt_render_frame_begin(self.h, C.byref(camera.c), C.c_void_p(d_f32 or None), C.c_void_p(d_u8 or None),
                                                  C.c_void_p(stream or None)), self._lib)

    def end_frame(self) -> Frame:
        st = abi.rt_stats()
        abi.check(self._lib.rt_render_frame_end(self.h, C.byref(st)), self._lib)
        return Frame.from_stats(None, None, st)

    def set_progressive(self, enable: bool) -> None:
        """rt_renderer_set_progressive: with it on, every frame also keeps each pixel's sums and RNG word (16 bytes per pixel), and
        continue_frame() adds samples to the last frame: a frame of a samples continued by b is the frame of a + b, bit for bit."""
        abi.check(self._lib.rt_renderer_set_progressive(self.h, int(bool(enable))), self._lib)

    @property
    def accumulated_samples(self) -> int:
        """Samples every pixel of the last frame holds (0: nothing to continue)."""
        n = C.c_uint32()
        abi.check(self._lib.rt_renderer_accumulated_samples(self.h, C.byref(n)), self._lib)
        return int(n.value)

    def continue_frame(self, samples: int, want_f32: bool = True, want_u8: bool = True) -> Frame:
        """rt_render_frame_continue: `samples` more samples for every pixel of the last frame, with its camera; the images are the mean
        over all the pixel's samples, the Frame's statistics (rays, launches, slices) those of this call."""
        rows, w = self.local_rows, self.img_size[0]
        f = np.zeros((rows, w, 4), np.float32) if want_f32 else None
        b = np.zeros((rows, w, 4), np.uint8) if want_u8 else None
        st = abi.rt_stats()
        abi.check(self._lib.rt_render_frame_continue(self.h, int(samples), abi.fptr(f) if want_f32 else None,
                                                     abi.u8ptr(b) if want_u8 else None, C.byref(st)), self._lib)
        return Frame.from_stats(f, b, st)

    def continue_frame_device(self, samples: int, d_f32: int = 0, d_u8: int = 0, stream: int = 0) -> Frame:
        """rt_render_frame_continue_device: as continue_frame, the outputs to DEVICE pointers; nothing is copied to host."""
        st = abi.rt_stats()
        abi.check(self._lib.rt_render_frame_continue_device(self.h, int(samples), C.c_void_p(d_f32 or None), C.c_void_p(d_u8 or None),
                                                            C.c_void_p(stream or None), C.byref(st)), self._lib)
        return Frame.from_stats(None, None, st)

    # ---- adaptive sampling (rt_mi355x.h): 8x8 blocks of the tile, tile-local row-major
    def block_grid(self) -> tuple[int, int]:
        """(blocks_x, blocks_y) = (ceil(W / 8), ceil(local_rows / 8))."""
        bx, by = C.c_uint32(), C.c_uint32()
        abi.check(self._lib.rt_renderer_block_grid(self.h, C.byref(bx), C.byref(by)), self._lib)
        return int(bx.value), int(by.value)

    def _n_blocks(self) -> int:
        bx, by = self.block_grid()
        return bx * by

    def continue_blocks(self, samples: int, blocks, want_f32: bool = True, want_u8: bool = True) -> Frame:
        """rt_render_frame_continue_blocks: `samples` more samples for the pixels of the listed blocks; the images are the tile's whole
        current image (every pixel over its own block's count), the Frame's statistics those of this call."""
        lst = np.ascontiguousarray(np.asarray(blocks, np.uint32).reshape(-1))
        rows, w = self.local_rows, self.img_size[0]
        f = np.zeros((rows, w, 4), np.float32) if want_f32 else None
        b = np.zeros((rows, w, 4), np.uint8) if want_u8 else None
        st = abi.rt_stats()
        abi.check(self._lib.rt_render_frame_continue_blocks(self.h, int(samples), lst.ctypes.data_as(C.POINTER(C.c_uint32)), int(lst.size),
                                                            abi.fptr(f) if want_f32 else None, abi.u8ptr(b) if want_u8 else None,
                                                            C.byref(st)), self._lib)
        return Frame.from_stats(f, b, st)

    def continue_blocks_device(self, samples: int, blocks, d_f32: int = 0, d_u8: int = 0, stream: int = 0) -> Frame:
        """rt_render_frame_continue_blocks_device: as continue_blocks, the outputs to DEVICE pointers (the list stays host memory)."""
        lst = np.ascontiguousarray(np.asarray(blocks, np.uint32).reshape(-1))
        st = abi.rt_stats()
        abi.check(self._lib.rt_render_frame_continue_blocks_device(self.h, int(samples), lst.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                                   int(lst.size), C.c_void_p(d_f32 or None), C.c_void_p(d_u8 or None),
                                                                   C.c_void_p(stream or None), C.byref(st)), self._lib)
        return Frame.from_stats(None, None, st)

    def adapt(self, threshold: float, min_samples: int = 0) -> np.ndarray:
        """rt_renderer_adapt: the active blocks, ascending (renders nothing)."""
        out = np.zeros(max(self._n_blocks(), 1), np.uint32)
        n = C.c_uint32()
        abi.check(self._lib.rt_renderer_adapt(self.h, float(threshold), int(min_samples), out.ctypes.data_as(C.POINTER(C.c_uint32)),
                                              C.byref(n)), self._lib)
        return out[:n.value].copy()

    def continue_adaptive(self, samples: int, threshold: float, min_samples: int = 0, want_f32: bool = True,
                          want_u8: bool = True) -> tuple[Frame, np.ndarray]:
        """rt_renderer_adapt + rt_render_frame_continue_blocks in one call (rt_render_frame_continue_adaptive): (Frame, the blocks it
        continued)."""
        blocks = self.adapt(threshold, min_samples)
        return self.continue_blocks(samples, blocks, want_f32, want_u8), blocks

    def continue_adaptive_c(self, samples: int, threshold: float, min_samples: int = 0, want_f32: bool = True,
                            want_u8: bool = True) -> tuple[Frame, int]:
        """rt_render_frame_continue_adaptive itself: (Frame, the number of blocks it continued)."""
        rows, w = self.local_rows, self.img_size[0]
        f = np.zeros((rows, w, 4), np.float32) if want_f32 else None
        b = np.zeros((rows, w, 4), np.uint8) if want_u8 else None
        st = abi.rt_stats()
        n = C.c_uint32()
        abi.check(self._lib.rt_render_frame_continue_adaptive(self.h, int(samples), float(threshold), int(min_samples),
                                                              abi.fptr(f) if want_f32 else None, abi.u8ptr(b) if want_u8 else None,
                                                              C.byref(st), C.byref(n)), self._lib)
        return Frame.from_stats(f, b, st), int(n.value)

    def continue_adaptive_device(self, samples: int, threshold: float, min_samples: int = 0, d_f32: int = 0, d_u8: int = 0,
                                 stream: int = 0) -> tuple[Frame, int]:
        """rt_render_frame_continue_adaptive_device: (Frame, the number of blocks it continued); outputs to DEVICE pointers."""
        st = abi.rt_stats()
        n = C.c_uint32()
        abi.check(self._lib.rt_render_frame_continue_adaptive_device(self.h, int(samples), float(threshold), int(min_samples),
                                                                     C.c_void_p(d_f32 or None), C.c_void_p(d_u8 or None),
                                                                     C.c_void_p(stream or None), C.byref(st), C.byref(n)), self._lib)
        return Frame.from_stats(None, None, st), int(n.value)

    def block_samples(self) -> np.ndarray:
        """Every block's sample count, (blocks_y, blocks_x) uint32 (zeros: nothing to continue)."""
        bx, by = self.block_grid()
        out = np.zeros(max(bx * by, 1), np.uint32)
        abi.check(self._lib.rt_renderer_block_samples(self.h, out.ctypes.data_as(C.POINTER(C.c_uint32))), self._lib)
        return out[:bx * by].reshape(by, bx)

    def block_errors(self) -> np.ndarray:
        """The last evaluation's e_B per block, (blocks_y, blocks_x) float32 (+inf: no snapshot)."""
        bx, by = self.block_grid()
        out = np.zeros(max(bx * by, 1), np.float32)
        abi.check(self._lib.rt_renderer_block_errors(self.h, out.ctypes.data_as(C.POINTER(C.c_float))), self._lib)
        return out[:bx * by].reshape(by, bx)

    def close(self):
        if self.h:
            self._lib.rt_renderer_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MegakernelRenderer(IRenderer):
    KIND = abi.RT_RENDERER_MEGAKERNEL


class WavefrontRenderer(IRenderer):
    KIND = abi.RT_RENDERER_WAVEFRONT


class TileComm:
    """One process driving several GPUs: the frame's interleaved strips are rendered by one renderer per device and brought to
    the root device by ONE grouped ncclGather over xGMI + a de-interleave kernel (rt_comm_create / rt_frame_gather in the C ABI;
    SURVEY §8e). With the same device listed more than once (a rehearsal of an N-GPU split on fewer GPUs) RCCL cannot be used
    (one rank per device) and the strips move by device copies instead: `uses_rccl` tells which."""

    def __init__(self, devices, lib=None):
        self._lib = lib or abi.load_library()
        self.devices = [int(d) for d in devices]
        arr = (C.c_int * len(self.devices))(*self.devices)
        self.h = C.c_void_p()
        abi.check(self._lib.rt_comm_create(len(self.devices), arr, C.byref(self.h)), self._lib)

    @property
    def uses_rccl(self) -> bool:
        return bool(self._lib.rt_comm_uses_rccl(self.h))

    def render_and_gather(self, renderers, camera: Camera, want_f32: bool = True, want_u8: bool = True):
        """renderers[i] = tile (i, n) on devices[i]. All tiles are enqueued (each into its renderer's own device buffers, no
        host copy), collected, gathered to the root and returned as (full rgba_f32 | None, full rgba_u8 | None, rays)."""
        n = len(self.devices)
        assert len(renderers) == n
        for r in renderers:
            r.begin_frame(camera, d_f32=self._lib.rt_renderer_tile_f32(r.h) if want_f32 else 0,
                          d_u8=self._lib.rt_renderer_tile_u8(r.h) if want_u8 else 0)
        rays = sum(r.end_frame().rays for r in renderers)
        w, h = renderers[0].img_size
        f = np.zeros((h, w, 4), np.float32) if want_f32 else None
        b = np.zeros((h, w, 4), np.uint8) if want_u8 else None
        hs = (C.c_void_p * n)(*[r.h for r in renderers])
        abi.check(self._lib.rt_frame_gather(self.h, hs, abi.fptr(f) if want_f32 else None, abi.u8ptr(b) if want_u8 else None, 0, 0), self._lib)
        return f, b, rays

    @property
    def size(self) -> int:
        return int(self._lib.rt_comm_size(self.h))

    def gather_begin(self, renderers, want_f32: bool = True, want_u8: bool = True) -> None:
        """rt_frame_gather_begin: enqueues the gather of the renderers' collected frames (no host wait); the renderers may begin their
        next frame right away."""
        hs = (C.c_void_p * len(renderers))(*[r.h for r in renderers])
        abi.check(self._lib.rt_frame_gather_begin(self.h, hs, int(want_f32), int(want_u8)), self._lib)

    def wait(self, shape, want_f32: bool = True, want_u8: bool = True):
        """rt_comm_wait: blocks until the gathered frame is complete on the root device and returns host copies of it."""
        h, w = shape
        f = np.zeros((h, w, 4), np.float32) if want_f32 else None
        b = np.zeros((h, w, 4), np.uint8) if want_u8 else None
        abi.check(self._lib.rt_comm_wait(self.h, abi.fptr(f) if want_f32 else None, abi.u8ptr(b) if want_u8 else None), self._lib)
        return f, b

    def close(self):
        if self.h:
            self._lib.rt_comm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# The lightmap filter's defaults (the image filter's, kept after scripts/lightmap_filter_probe.py's sweep). sigma_position is
# LIGHTMAP_POSITION_FRACTION of the scene's scale (Scene.scale()).
LIGHTMAP_FILTER_ITERATIONS = 5
LIGHTMAP_SIGMA_LUMINANCE = 4.0
LIGHTMAP_SIGMA_NORMAL = 0.25
LIGHTMAP_POSITION_FRACTION = 0.05


def lightmap_filter_params(iterations: int = LIGHTMAP_FILTER_ITERATIONS, sigma_luminance: float = LIGHTMAP_SIGMA_LUMINANCE,
                           sigma_normal: float = LIGHTMAP_SIGMA_NORMAL, sigma_position: float | None = None, scene_scale: float | None = None):
    """rt_lightmap_filter_params; sigma_position None: LIGHTMAP_POSITION_FRACTION * scene_scale, in fp32 (scene_scale is then required)."""
    if sigma_position is None:
        if scene_scale is None:
            raise ValueError("give sigma_position or scene_scale (Scene.scale())")
        sigma_position = float(np.float32(LIGHTMAP_POSITION_FRACTION) * np.float32(scene_scale))
    return abi.rt_lightmap_filter_params(int(iterations), float(sigma_luminance), float(sigma_normal), float(sigma_position))


class Lightmap:
    """rt_lightmap: a width x height lightmap atlas over `scene` (include/rt_mi355x.h: rt_lightmap_bake). lm_uv: (T, 3, 2) or (T, 6)
    float32, every triangle's three lightmap UVs in the scene's triangle order (rtamd.bake.triangle_grid_uvs makes a trivial unwrap).
    max_repeats: the most entries per texel a bake may ask for. filter=True (RT_LIGHTMAP_FILTER): also bake_filtered and filter. Close it
    before its scene."""

    def __init__(self, scene: Scene, lm_uv: np.ndarray, width: int, height: int, max_repeats: int = 1, filter: bool = False):
        lm_uv = np.asarray(lm_uv)
        t = scene.desc.n_triangles
        if lm_uv.shape not in ((t, 3, 2), (t, 6)):
            raise ValueError(f"lm_uv must hold three (u, v) per triangle, shape ({t}, 3, 2) or ({t}, 6), got {lm_uv.shape}")
        if lm_uv.dtype.kind != "f":
            raise ValueError("lm_uv must be a floating-point array")
        self._uv = np.ascontiguousarray(lm_uv, np.float32)
        self._lib = scene._lib
        self.scene = scene
        self.width, self.height, self.max_repeats = int(width), int(height), int(max_repeats)
        self.h = C.c_void_p()
        if filter:
            abi.check(self._lib.rt_lightmap_create_ex(scene.h, self.width, self.height, self.max_repeats, abi.fptr(self._uv),
                                                      abi.RT_LIGHTMAP_FILTER, C.byref(self.h)), self._lib)
        else:
            abi.check(self._lib.rt_lightmap_create(scene.h, self.width, self.height, self.max_repeats, abi.fptr(self._uv), C.byref(self.h)),
                      self._lib)

    def texels(self) -> dict:
        """rt_lightmap_texels: {"tri": (H, W) uint32, the owning triangle or 0xFFFFFFFF, "pos": (H, W, 3) float32, the texel centre's point on
        it (NaN where empty), "normal": (H, W, 3) float32, its shading normal there (0 where empty)}."""
        out = {"tri": np.zeros((self.height, self.width), np.uint32), "pos": np.zeros((self.height, self.width, 3), np.float32),
               "normal": np.zeros((self.height, self.width, 3), np.float32)}
        abi.check(self._lib.rt_lightmap_texels(self.h, abi.u32ptr(out["tri"]), abi.fptr(out["pos"]), abi.fptr(out["normal"])), self._lib)
        return out

    def texels_device(self, d_tri: int = 0, d_pos: int = 0, d_normal: int = 0, stream: int = 0) -> None:
        """rt_lightmap_texels_device on DEVICE pointers (e.g. torch .data_ptr()), enqueued on `stream`; 0 = NULL (not written)."""
        v = [C.c_void_p(x or None) for x in (d_tri, d_pos, d_normal, stream)]
        abi.check(self._lib.rt_lightmap_texels_device(self.h, *v), self._lib)

    def bake(self, samples: int, max_depth: int, seed: int, repeats: int = 1, rr_start: int = 0, dilate: int = 0) -> dict:
        """rt_lightmap_bake: {"rgba": (H, W, 4) float32, the gathered radiance with alpha 1 where sampled, 0.5 where filled by dilation, 0
        where empty, "stats": {"covered", "sampled", "filled", "rays"}}. samples x repeats paths per texel; `dilate` gutter passes."""
        p = abi.rt_lightmap_params(int(samples), int(max_depth), int(rr_start), int(repeats), int(seed) & 0xFFFFFFFF, int(dilate))
        rgba = np.zeros((self.height, self.width, 4), np.float32)
        st = abi.rt_lightmap_stats()
        abi.check(self._lib.rt_lightmap_bake(self.h, C.byref(p), abi.fptr(rgba), C.byref(st)), self._lib)
        return {"rgba": rgba, "stats": {"covered": st.covered, "sampled": st.sampled, "filled": st.filled, "rays": st.rays}}

    def bake_device(self, d_rgba: int, samples: int, max_depth: int, seed: int, repeats: int = 1, rr_start: int = 0, dilate: int = 0,
                    d_stats: int = 0, stream: int = 0) -> None:
        """rt_lightmap_bake_device on DEVICE pointers, enqueued on `stream`: d_rgba H*W*4 floats, d_stats 24 bytes (rt_lightmap_stats) or 0."""
        p = abi.rt_lightmap_params(int(samples), int(max_depth), int(rr_start), int(repeats), int(seed) & 0xFFFFFFFF, int(dilate))
        abi.check(self._lib.rt_lightmap_bake_device(self.h, C.byref(p), C.c_void_p(d_rgba or None), C.c_void_p(d_stats or None),
                                                    C.c_void_p(stream or None)), self._lib)

    def _filter_params(self, params: dict):
        """lightmap_filter_params(**params), sigma_position a fraction of the lightmap's scene where neither it nor scene_scale is given"""
        if params.get("sigma_position") is None and params.get("scene_scale") is None:
            params = dict(params, scene_scale=self.scene.scale())
        return lightmap_filter_params(**params)

    def bake_filtered(self, samples: int, max_depth: int, seed: int, repeats: int = 2, rr_start: int = 0, dilate: int = 0,
                      want_variance: bool = True, **params) -> dict:
        """rt_lightmap_bake_filtered: bake()'s dictionary with the plane filtered in front of the dilation, and "variance": (H, W) float32,
        the variance of each sampled texel's mean luminance after the filter (None if not wanted). `params`: lightmap_filter_params'."""
        f = self._filter_params(params)
        p = abi.rt_lightmap_params(int(samples), int(max_depth), int(rr_start), int(repeats), int(seed) & 0xFFFFFFFF, int(dilate))
        rgba = np.zeros((self.height, self.width, 4), np.float32)
        var = np.zeros((self.height, self.width), np.float32) if want_variance else None
        st = abi.rt_lightmap_stats()
        abi.check(self._lib.rt_lightmap_bake_filtered(self.h, C.byref(p), C.byref(f), abi.fptr(rgba), abi.fptr(var) if want_variance else None,
                                                      C.byref(st)), self._lib)
        return {"rgba": rgba, "variance": var, "stats": {"covered": st.covered, "sampled": st.sampled, "filled": st.filled, "rays": st.rays}}

    def bake_filtered_device(self, d_rgba: int, samples: int, max_depth: int, seed: int, repeats: int = 2, rr_start: int = 0, dilate: int = 0,
                             d_variance: int = 0, d_stats: int = 0, stream: int = 0, **params) -> None:
        """rt_lightmap_bake_filtered_device on DEVICE pointers, enqueued on `stream`: d_rgba H*W*4 floats, d_variance H*W floats or 0, d_stats
        24 bytes or 0."""
        f = self._filter_params(params)
        p = abi.rt_lightmap_params(int(samples), int(max_depth), int(rr_start), int(repeats), int(seed) & 0xFFFFFFFF, int(dilate))
        v = [C.c_void_p(x or None) for x in (d_rgba, d_variance, d_stats, stream)]
        abi.check(self._lib.rt_lightmap_bake_filtered_device(self.h, C.byref(p), C.byref(f), *v), self._lib)

    def filter(self, rgba: np.ndarray, variance: np.ndarray | None, want_variance: bool = True, out_rgba: np.ndarray | None = None,
               **params) -> dict:
        """rt_lightmap_filter of a (H, W, 4) float32 plane (alpha 1 = a texel to filter) with the (H, W) float32 variance of its luminance
        (None: only with sigma_luminance = inf), guided by the lightmap's own texels: {"rgba", "variance"} (None if not wanted). out_rgba:
        where the result goes (may be rgba). `params`: lightmap_filter_params'."""
        shape = (self.height, self.width, 4)
        planes = [("rgba", rgba, shape)]
        if variance is not None:
            planes.append(("variance", variance, shape[:2]))
        if out_rgba is not None:
            planes.append(("out_rgba", out_rgba, shape))
        for name, a, want in planes:
            if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.shape != want or not a.flags.c_contiguous:
                raise ValueError(f"{name} must be a C-contiguous float32 array of shape {want}")
        f = self._filter_params(params)
        out = np.zeros(shape, np.float32) if out_rgba is None else out_rgba
        var = np.zeros(shape[:2], np.float32) if want_variance else None
        abi.check(self._lib.rt_lightmap_filter(self.h, C.byref(f), abi.fptr(rgba), abi.fptr(variance) if variance is not None else None,
                                               abi.fptr(out), abi.fptr(var) if want_variance else None), self._lib)
        return {"rgba": out, "variance": var}

    def filter_device(self, d_rgba: int, d_variance: int, d_out_rgba: int, d_out_variance: int = 0, stream: int = 0, **params) -> None:
        """rt_lightmap_filter_device on DEVICE pointers, enqueued on `stream`; d_variance 0 only with sigma_luminance = inf."""
        f = self._filter_params(params)
        v = [C.c_void_p(x or None) for x in (d_rgba, d_variance, d_out_rgba, d_out_variance, stream)]
        abi.check(self._lib.rt_lightmap_filter_device(self.h, C.byref(f), *v), self._lib)

    def close(self):
        if self.h:
            self._lib.rt_lightmap_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ProbeVolume:
    """rt_probe_volume: a count[0] x count[1] x count[2] grid of irradiance probes over `scene`, nine spherical-harmonic coefficients each
    (include/rt_mi355x.h: rt_probe_volume_bake). Probe (ix, iy, iz) sits at origin + (ix, iy, iz) * spacing; `spacing` is one number or one
    per axis. max_dirs: the most directions per probe a bake may ask for (rtamd.bake.probe_grid fits origin and count to a scene). A table
    is (probes, 9, 4) float32, probe index (iz * count[1] + iy) * count[0] + ix, validity in [:, 0, 3]. Close it before its scene."""

    def __init__(self, scene: Scene, origin, spacing, count, max_dirs: int = 64):
        origin, count = np.asarray(origin, np.float64), np.asarray(count)
        spacing = np.asarray(spacing, np.float64)
        if spacing.ndim == 0:
            spacing = np.repeat(spacing, 3)
        if origin.shape != (3,) or spacing.shape != (3,):
            raise ValueError("origin must hold 3 numbers, spacing 1 or 3")
        if count.shape != (3,) or count.dtype.kind not in "ui":
            raise ValueError("count must hold 3 integers")
        if (count < 0).any() or (count > 0xFFFFFFFF).any() or not 0 <= int(max_dirs) <= 0xFFFFFFFF:
            raise ValueError("count and max_dirs must fit 32 unsigned bits")
        self._lib = scene._lib
        self.scene = scene
        self.desc = abi.rt_probe_volume_desc((C.c_float * 3)(*origin), (C.c_float * 3)(*spacing), (C.c_uint32 * 3)(*[int(c) for c in count]),
                                             int(max_dirs))
        self.origin, self.spacing = np.array(list(self.desc.origin), np.float32), np.array(list(self.desc.spacing), np.float32)
        self.count, self.max_dirs = tuple(int(c) for c in count), int(max_dirs)
        self.probes = self.count[0] * self.count[1] * self.count[2]
        self.h = C.c_void_p()
        abi.check(self._lib.rt_probe_volume_create(scene.h, C.byref(self.desc), 0, C.byref(self.h)), self._lib)

    @staticmethod
    def _params(dirs, max_depth, rr_start, seed):
        return abi.rt_probe_bake_params(int(dirs), int(max_depth), int(rr_start), int(seed) & 0xFFFFFFFF)

    def positions(self) -> np.ndarray:
        """The probes' positions, (probes, 3) float32, in the contract's arithmetic (one fp32 multiply and one add per axis)."""
        iz, iy, ix = np.meshgrid(*(np.arange(c) for c in self.count[::-1]), indexing="ij")
        idx = np.stack([ix, iy, iz], -1).reshape(-1, 3).astype(np.float32)
        return self.origin[None, :] + idx * self.spacing[None, :]

    def entries(self, dirs: int, seed: int) -> dict:
        """rt_probe_volume_entries: {"pos": (probes * dirs, 3) float32, "dir": (probes * dirs, 3) float32, the uniform directions, "state":
        (probes * dirs,) uint32, the states the paths start with}, entry e = p * dirs + j."""
        n = self.probes * max(int(dirs), 0)
        out = {"pos": np.zeros((n, 3), np.float32), "dir": np.zeros((n, 3), np.float32), "state": np.zeros(n, np.uint32)}
        p = self._params(dirs, 1, 0, seed)
        abi.check(self._lib.rt_probe_volume_entries(self.h, C.byref(p), abi.fptr(out["pos"]), abi.fptr(out["dir"]), abi.u32ptr(out["state"])),
                  self._lib)
        return out

    def entries_device(self, dirs: int, seed: int, d_pos: int = 0, d_dir: int = 0, d_state: int = 0, stream: int = 0) -> None:
        """rt_probe_volume_entries_device on DEVICE pointers (e.g. torch .data_ptr()), enqueued on `stream`; 0 = NULL (not written)."""
        p = self._params(dirs, 1, 0, seed)
        v = [C.c_void_p(x or None) for x in (d_pos, d_dir, d_state, stream)]
        abi.check(self._lib.rt_probe_volume_entries_device(self.h, C.byref(p), *v), self._lib)

    def bake(self, dirs: int, max_depth: int, rr_start: int = 0, seed: int = 0):
        """rt_probe_volume_bake -> (sh (probes, 9, 4) float32, {"probes", "valid", "rays"}); the table also stays in the volume."""
        p = self._params(dirs, max_depth, rr_start, seed)
        sh = np.zeros((self.probes, 9, 4), np.float32)
        st = abi.rt_probe_stats()
        abi.check(self._lib.rt_probe_volume_bake(self.h, C.byref(p), abi.fptr(sh), C.byref(st)), self._lib)
        return sh, {"probes": st.probes, "valid": st.valid, "rays": st.rays}

    def bake_device(self, dirs: int, max_depth: int, rr_start: int = 0, seed: int = 0, d_sh: int = 0, d_stats: int = 0, stream: int = 0) -> None:
        """rt_probe_volume_bake_device, enqueued on `stream`: d_sh probes * 36 floats or 0, d_stats 16 bytes (rt_probe_stats) or 0."""
        p = self._params(dirs, max_depth, rr_start, seed)
        v = [C.c_void_p(x or None) for x in (d_sh, d_stats, stream)]
        abi.check(self._lib.rt_probe_volume_bake_device(self.h, C.byref(p), *v), self._lib)

    def set_sh(self, sh: np.ndarray) -> None:
        """rt_probe_volume_set_sh: load a (probes, 9, 4) float32 table (a saved bake, or a synthetic one)."""
        if not isinstance(sh, np.ndarray) or sh.dtype != np.float32 or sh.shape != (self.probes, 9, 4):
            raise ValueError(f"sh must be a float32 array of shape ({self.probes}, 9, 4)")
        sh = np.ascontiguousarray(sh)
        abi.check(self._lib.rt_probe_volume_set_sh(self.h, abi.fptr(sh)), self._lib)

    def set_sh_device(self, d_sh: int, stream: int = 0) -> None:
        abi.check(self._lib.rt_probe_volume_set_sh_device(self.h, C.c_void_p(d_sh or None), C.c_void_p(stream or None)), self._lib)

    def get_sh(self) -> np.ndarray:
        sh = np.zeros((self.probes, 9, 4), np.float32)
        abi.check(self._lib.rt_probe_volume_get_sh(self.h, abi.fptr(sh)), self._lib)
        return sh

    def get_sh_device(self, d_sh: int, stream: int = 0) -> None:
        abi.check(self._lib.rt_probe_volume_get_sh_device(self.h, C.c_void_p(d_sh or None), C.c_void_p(stream or None)), self._lib)

    def sample(self, pos: np.ndarray, normal: np.ndarray) -> np.ndarray:
        """rt_probe_volume_sample: pos, normal (n, 3) -> (n, 3) float32, irradiance over pi at the points for those normals (used as
        given): what a white Lambertian surface there would scatter."""
        pos, normal = np.asarray(pos), np.asarray(normal)
        if pos.ndim != 2 or pos.shape[1] != 3 or normal.shape != pos.shape:
            raise ValueError("pos and normal must both be (n, 3)")
        if pos.dtype.kind != "f" or normal.dtype.kind != "f":
            raise ValueError("pos and normal must be floating-point arrays")
        pos, normal = np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(normal, np.float32)
        out = np.zeros(pos.shape, np.float32)
        abi.check(self._lib.rt_probe_volume_sample(self.h, pos.shape[0], abi.fptr(pos), abi.fptr(normal), abi.fptr(out)), self._lib)
        return out

    def sample_device(self, n: int, d_pos: int, d_normal: int, d_rgb: int, stream: int = 0) -> None:
        """rt_probe_volume_sample_device on DEVICE pointers, 3n floats each, enqueued on `stream`."""
        v = [C.c_void_p(x or None) for x in (d_pos, d_normal, d_rgb, stream)]
        abi.check(self._lib.rt_probe_volume_sample_device(self.h, int(n), *v), self._lib)

    def close(self):
        if self.h:
            self._lib.rt_probe_volume_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ReflectionProbes:
    """rt_reflection_probes: cube-map captures at `positions` (count, 3) over `scene`, each a chain of `levels` levels with faces of
    size >> l texels, prefiltered for growing roughness (include/rt_mi355x.h: rt_reflection_probes_bake). boxes: None, or (count, 6), min then
    max per probe, the parallax boxes of sample. max_spt: the most samples per level-0 texel a bake may ask for. A chain is
    (count, chain_texels, 4) float32, level l of a probe at [level_offset(l) : level_offset(l + 1)] as (6, S_l, S_l, 4), validity in .w
    (rtamd.bake.lod_for_roughness and reflect_dirs give sample's lod and direction). Close it before its scene."""

    def __init__(self, scene: Scene, positions, size: int, levels: int, max_spt: int = 1, boxes=None):
        pos = np.asarray(positions)
        if pos.ndim != 2 or pos.shape[1] != 3 or pos.dtype.kind not in "fiu":
            raise ValueError("positions must be (count, 3) numbers")
        if boxes is not None:
            boxes = np.asarray(boxes)
            if boxes.shape != (pos.shape[0], 6) or boxes.dtype.kind not in "fiu":
                raise ValueError("boxes must be (count, 6) numbers: min then max per probe")
        for v in (size, levels, max_spt):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError("size, levels and max_spt must fit 32 unsigned bits")
        self._lib = scene._lib
        self.scene = scene
        self.positions = np.ascontiguousarray(pos, np.float32)
        self.boxes = None if boxes is None else np.ascontiguousarray(boxes, np.float32)
        self.count, self.size, self.levels, self.max_spt = int(pos.shape[0]), int(size), int(levels), int(max_spt)
        self.face0 = 6 * self.size * self.size
        self.chain_texels = sum(6 * (self.size >> l) ** 2 for l in range(self.levels))
        self.desc = abi.rt_reflection_probes_desc(self.count, self.size, self.levels, self.max_spt, abi.fptr(self.positions),
                                                  abi.fptr(self.boxes) if self.boxes is not None else None)
        self.h = C.c_void_p()
        abi.check(self._lib.rt_reflection_probes_create(scene.h, C.byref(self.desc), 0, C.byref(self.h)), self._lib)

    @staticmethod
    def _params(spt, max_depth, rr_start, seed, clamp):
        return abi.rt_reflection_bake_params(int(spt), int(max_depth), int(rr_start), int(seed) & 0xFFFFFFFF, float(clamp))

    def level_offset(self, l: int) -> int:
        """The texels of a probe's chain in front of level l (l == levels: the chain's length)."""
        return sum(6 * (self.size >> m) ** 2 for m in range(int(l)))

    def level(self, chain: np.ndarray, l: int) -> np.ndarray:
        """Level l of every probe of a chain, (count, 6, S_l, S_l, 4): a view."""
        S = self.size >> int(l)
        return chain[:, self.level_offset(l):self.level_offset(l + 1)].reshape(self.count, 6, S, S, 4)

    def entries(self, spt: int, seed: int) -> dict:
        """rt_reflection_probes_entries: {"pos", "dir": (entries, 3) float32, the probes' positions and the jittered face directions, "state":
        (entries,) uint32, the states the paths start with}, entry e = (((p * 6 + f) * size + y) * size + x) * spt + j."""
        n = self.count * self.face0 * max(int(spt), 0)
        out = {"pos": np.zeros((n, 3), np.float32), "dir": np.zeros((n, 3), np.float32), "state": np.zeros(n, np.uint32)}
        p = self._params(spt, 1, 0, seed, 0.0)
        abi.check(self._lib.rt_reflection_probes_entries(self.h, C.byref(p), abi.fptr(out["pos"]), abi.fptr(out["dir"]), abi.u32ptr(out["state"])),
                  self._lib)
        return out

    def entries_device(self, spt: int, seed: int, d_pos: int = 0, d_dir: int = 0, d_state: int = 0, stream: int = 0) -> None:
        """rt_reflection_probes_entries_device on DEVICE pointers (e.g. torch .data_ptr()), enqueued on `stream`; 0 = NULL (not written)."""
        p = self._params(spt, 1, 0, seed, 0.0)
        v = [C.c_void_p(x or None) for x in (d_pos, d_dir, d_state, stream)]
        abi.check(self._lib.rt_reflection_probes_entries_device(self.h, C.byref(p), *v), self._lib)

    def bake(self, spt: int, max_depth: int, rr_start: int = 0, seed: int = 0, clamp: float = 0.0):
        """rt_reflection_probes_bake -> (chain (count, chain_texels, 4) float32, {"probes", "valid", "rays"}); the chain also stays in the object."""
        p = self._params(spt, max_depth, rr_start, seed, clamp)
        chain = np.zeros((self.count, self.chain_texels, 4), np.float32)
        st = abi.rt_reflection_stats()
        abi.check(self._lib.rt_reflection_probes_bake(self.h, C.byref(p), abi.fptr(chain), C.byref(st)), self._lib)
        return chain, {"probes": st.probes, "valid": st.valid, "rays": st.rays}

    def bake_device(self, spt: int, max_depth: int, rr_start: int = 0, seed: int = 0, clamp: float = 0.0, d_chain: int = 0, d_stats: int = 0,
                    stream: int = 0) -> None:
        """rt_reflection_probes_bake_device, enqueued on `stream`: d_chain count * chain_texels * 4 floats or 0, d_stats 16 bytes or 0."""
        p = self._params(spt, max_depth, rr_start, seed, clamp)
        v = [C.c_void_p(x or None) for x in (d_chain, d_stats, stream)]
        abi.check(self._lib.rt_reflection_probes_bake_device(self.h, C.byref(p), *v), self._lib)

    def set_level0(self, level0: np.ndarray) -> None:
        """rt_reflection_probes_set_level0: load a (count, 6, size, size, 4) float32 level 0 (a saved capture, or a synthetic one); the levels
        above it are stale until prefilter()."""
        if not isinstance(level0, np.ndarray) or level0.dtype != np.float32 or level0.shape != (self.count, 6, self.size, self.size, 4):
            raise ValueError(f"level0 must be a float32 array of shape ({self.count}, 6, {self.size}, {self.size}, 4)")
        level0 = np.ascontiguousarray(level0)
        abi.check(self._lib.rt_reflection_probes_set_level0(self.h, abi.fptr(level0)), self._lib)

    def set_level0_device(self, d_level0: int, stream: int = 0) -> None:
        abi.check(self._lib.rt_reflection_probes_set_level0_device(self.h, C.c_void_p(d_level0 or None), C.c_void_p(stream or None)), self._lib)

    def prefilter(self) -> None:
        """rt_reflection_probes_prefilter: the levels above 0 from the level 0 held."""
        abi.check(self._lib.rt_reflection_probes_prefilter(self.h), self._lib)

    def prefilter_device(self, stream: int = 0) -> None:
        abi.check(self._lib.rt_reflection_probes_prefilter_device(self.h, C.c_void_p(stream or None)), self._lib)

    def get_chain(self) -> np.ndarray:
        chain = np.zeros((self.count, self.chain_texels, 4), np.float32)
        abi.check(self._lib.rt_reflection_probes_get_chain(self.h, abi.fptr(chain)), self._lib)
        return chain

    def get_chain_device(self, d_chain: int, stream: int = 0) -> None:
        abi.check(self._lib.rt_reflection_probes_get_chain_device(self.h, C.c_void_p(d_chain or None), C.c_void_p(stream or None)), self._lib)

    def sample(self, probe_index: np.ndarray, dirs: np.ndarray, lod, pos=None) -> np.ndarray:
        """rt_reflection_probes_sample: probe_index (n,) integers, dirs (n, 3), lod (n,) or one number, pos None or (n, 3) (with boxes: the
        parallax correction) -> (n, 3) float32, the radiance along the directions."""
        idx, dirs = np.asarray(probe_index), np.asarray(dirs)
        if dirs.ndim != 2 or dirs.shape[1] != 3 or dirs.dtype.kind != "f":
            raise ValueError("dirs must be a floating-point (n, 3) array")
        n = dirs.shape[0]
        if idx.shape != (n,) or idx.dtype.kind not in "ui" or (n and (idx.min() < 0 or idx.max() > 0xFFFFFFFF)):
            raise ValueError("probe_index must be (n,) integers that fit 32 unsigned bits")
        lod = np.asarray(lod)
        if lod.ndim == 0:
            lod = np.repeat(lod, n)
        if lod.shape != (n,) or lod.dtype.kind not in "fiu":
            raise ValueError("lod must be one number or (n,) numbers")
        if pos is not None:
            pos = np.asarray(pos)
            if pos.shape != dirs.shape or pos.dtype.kind != "f":
                raise ValueError("pos must be a floating-point (n, 3) array, as dirs")
            pos = np.ascontiguousarray(pos, np.float32)
        idx, dirs, lod = np.ascontiguousarray(idx, np.uint32), np.ascontiguousarray(dirs, np.float32), np.ascontiguousarray(lod, np.float32)
        out = np.zeros((n, 3), np.float32)
        abi.check(self._lib.rt_reflection_probes_sample(self.h, n, abi.u32ptr(idx), abi.fptr(pos) if pos is not None else None, abi.fptr(dirs),
                                                        abi.fptr(lod), abi.fptr(out)), self._lib)
        return out

    def sample_device(self, n: int, d_index: int, d_pos: int, d_dir: int, d_lod: int, d_rgb: int, stream: int = 0) -> None:
        """rt_reflection_probes_sample_device on DEVICE pointers (d_pos 0 = NULL: no parallax correction), enqueued on `stream`."""
        v = [C.c_void_p(x or None) for x in (d_index, d_pos, d_dir, d_lod, d_rgb, stream)]
        abi.check(self._lib.rt_reflection_probes_sample_device(self.h, int(n), *v), self._lib)

    def close(self):
        if self.h:
            self._lib.rt_reflection_probes_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# The denoiser's defaults (chosen by scripts/denoise_probe.py's sweep on the atrium and the Cornell box). sigma_position is
# DENOISE_POSITION_FRACTION of the scene's scale (Scene.scale()); host/main.cpp's --denoise uses the same values.
DENOISE_ITERATIONS = 5
DENOISE_SIGMA_COLOR = 1.0
DENOISE_SIGMA_NORMAL = 0.25
DENOISE_POSITION_FRACTION = 0.05
DENOISE_SIGMA_ALBEDO = 0.1
# The variance-guided filter's: the luminance tolerance in standard deviations, and the history length from which the temporal
# moments are trusted; one setting for every scene. host/main.cpp's --guided uses the same min_history.
DENOISE_SIGMA_LUMINANCE = 4.0
DENOISE_MIN_HISTORY = 4


def _float_planes(shape, *arrays):
    """The arrays as contiguous float32, each of `shape`."""
    out = [np.ascontiguousarray(a, np.float32) for a in arrays]
    for a in out:
        if a.shape != shape:
            raise ValueError(f"expected {shape}, got {a.shape}")
    return out


def _outputs(shape, want_f32, want_u8, out_f32):
    """(f32, u8) a host call writes: fresh (or out_f32) where asked for, else None; and their pointers (None: not asked for)."""
    f = (out_f32 if out_f32 is not None else np.zeros(shape, np.float32)) if want_f32 else None
    b = np.zeros(shape, np.uint8) if want_u8 else None
    return f, b, (abi.fptr(f) if f is not None else None, abi.u8ptr(b) if b is not None else None)


def _sigma_position(sigma_position, fraction, scene_scale, missing):
    """sigma_position, or `fraction` of the scene's scale in fp32 where it is None (`missing`: the caller's words where both are)."""
    if sigma_position is not None:
        return float(sigma_position)
    if scene_scale is None:
        raise ValueError(missing)
    return float(np.float32(fraction) * np.float32(scene_scale))


def denoise_params(iterations: int = DENOISE_ITERATIONS, sigma_color: float = DENOISE_SIGMA_COLOR, sigma_normal: float = DENOISE_SIGMA_NORMAL,
                   sigma_position: float | None = None, sigma_albedo: float = DENOISE_SIGMA_ALBEDO, scene_scale: float | None = None):
    """rt_denoise_params; sigma_position None: DENOISE_POSITION_FRACTION * scene_scale, in fp32 (scene_scale is then required)."""
    sp = _sigma_position(sigma_position, DENOISE_POSITION_FRACTION, scene_scale, "give sigma_position or scene_scale (Scene.scale())")
    return abi.rt_denoise_params(int(iterations), float(sigma_color), float(sigma_normal), sp, float(sigma_albedo))


def denoise_var_params(iterations: int = DENOISE_ITERATIONS, sigma_luminance: float = DENOISE_SIGMA_LUMINANCE,
                       sigma_normal: float = DENOISE_SIGMA_NORMAL, sigma_position: float | None = None, sigma_albedo: float = DENOISE_SIGMA_ALBEDO,
                       min_history: int = DENOISE_MIN_HISTORY, scene_scale: float | None = None):
    """rt_denoise_var_params; sigma_position None: DENOISE_POSITION_FRACTION * scene_scale, in fp32 (scene_scale is then required)."""
    sp = _sigma_position(sigma_position, DENOISE_POSITION_FRACTION, scene_scale, "give sigma_position or scene_scale (Scene.scale())")
    return abi.rt_denoise_var_params(int(iterations), float(sigma_luminance), float(sigma_normal), sp, float(sigma_albedo), int(min_history))


class Denoiser:
    """rt_denoiser: the edge-avoiding a-trous filter for W x H frames on one device, guided by Scene.gbuffer's planes. variance=True
    (RT_DENOISER_VARIANCE): also the variance estimate and the variance-guided filter."""

    def __init__(self, device: int, width: int, height: int, lib=None, variance: bool = False):
        self._lib = lib or abi.load_library()
        self.width, self.height = int(width), int(height)
        self.h = C.c_void_p()
        if variance:
            abi.check(self._lib.rt_denoiser_create_ex(int(device), self.width, self.height, abi.RT_DENOISER_VARIANCE, C.byref(self.h)), self._lib)
        else:
            abi.check(self._lib.rt_denoiser_create(int(device), self.width, self.height, C.byref(self.h)), self._lib)

    def denoise(self, frame_f32: np.ndarray, gbuf: dict, iterations: int = DENOISE_ITERATIONS, want_f32: bool = True, want_u8: bool = True,
                out_f32: np.ndarray | None = None, **sigmas):
        """rt_denoise of a (H, W, 4) float32 frame; returns (f32, u8), None for a plane not asked for. `sigmas`: sigma_color,
        sigma_normal, sigma_position, sigma_albedo, scene_scale (denoise_params). out_f32: where the fp32 result goes (may be frame_f32)."""
        p = denoise_params(iterations, **sigmas)
        planes = self._planes(frame_f32, gbuf)
        f, b, out = _outputs(planes[0].shape, want_f32, want_u8, out_f32)
        abi.check(self._lib.rt_denoise(self.h, C.byref(p), *(abi.fptr(a) for a in planes), *out), self._lib)
        return f, b

    def denoise_device(self, d_frame: int, d_albedo: int, d_normal: int, d_position: int, d_out_f32: int = 0, d_out_u8: int = 0,
                       stream: int = 0, iterations: int = DENOISE_ITERATIONS, **sigmas) -> None:
        """rt_denoise_device on DEVICE pointers (e.g. torch .data_ptr()), enqueued on `stream`."""
        p = denoise_params(iterations, **sigmas)
        v = [C.c_void_p(x or None) for x in (d_frame, d_albedo, d_normal, d_position, d_out_f32, d_out_u8, stream)]
        abi.check(self._lib.rt_denoise_device(self.h, C.byref(p), *v), self._lib)

    def _planes(self, frame_f32, gbuf):
        """the four input planes of a host call, checked: the frame, albedo, normal, position"""
        return _float_planes((self.height, self.width, 4), frame_f32, gbuf["albedo"], gbuf["normal"], gbuf["position"])

    def estimate_variance(self, frame_f32: np.ndarray, gbuf: dict, moments: np.ndarray | None = None, history_len: np.ndarray | None = None,
                          **params) -> np.ndarray:
        """rt_denoise_variance: the (H, W) float32 variance of the frame's luminance; moments (H, W, 2) and history_len (H, W) as
        TemporalAccumulator.accumulate(moments=True) returns them, or neither (a still image). `params`: denoise_var_params'."""
        p = denoise_var_params(**params)
        planes = self._planes(frame_f32, gbuf)
        m = n = None
        if moments is not None:
            m = np.ascontiguousarray(moments, np.float32)
            if m.shape != (self.height, self.width, 2):
                raise ValueError(f"expected moments of shape {(self.height, self.width, 2)}, got {m.shape}")
        if history_len is not None:
            n = np.ascontiguousarray(history_len, np.float32)
            if n.shape != (self.height, self.width):
                raise ValueError(f"expected history_len of shape {(self.height, self.width)}, got {n.shape}")
        var = np.zeros((self.height, self.width), np.float32)
        abi.check(self._lib.rt_denoise_variance(self.h, C.byref(p), *(abi.fptr(a) for a in planes),
                                                abi.fptr(m) if m is not None else None, abi.fptr(n) if n is not None else None,
                                                abi.fptr(var)), self._lib)
        return var

    def estimate_variance_device(self, d_frame: int, d_albedo: int, d_normal: int, d_position: int, d_moments: int, d_history_len: int,
                                 d_out_variance: int, stream: int = 0, **params) -> None:
        """rt_denoise_variance_device on DEVICE pointers, enqueued on `stream`."""
        p = denoise_var_params(**params)
        v = [C.c_void_p(x or None) for x in (d_frame, d_albedo, d_normal, d_position, d_moments, d_history_len, d_out_variance, stream)]
        abi.check(self._lib.rt_denoise_variance_device(self.h, C.byref(p), *v), self._lib)

    def denoise_guided(self, frame_f32: np.ndarray, gbuf: dict, variance: np.ndarray, iterations: int = DENOISE_ITERATIONS, want_f32: bool = True,
                       want_u8: bool = True, want_variance: bool = True, out_f32: np.ndarray | None = None, **params):
        """rt_denoise_guided of a (H, W, 4) float32 frame with its (H, W) variance; returns (f32, u8, variance of the result), None for what
        was not asked for. `params`: denoise_var_params'. out_f32: where the fp32 result goes (may be frame_f32)."""
        p = denoise_var_params(iterations, **params)
        planes = self._planes(frame_f32, gbuf)
        variance = np.ascontiguousarray(variance, np.float32)
        if variance.shape != (self.height, self.width):
            raise ValueError(f"expected variance of shape {(self.height, self.width)}, got {variance.shape}")
        f, b, out = _outputs(planes[0].shape, want_f32, want_u8, out_f32)
        ov = np.zeros(variance.shape, np.float32) if want_variance else None
        abi.check(self._lib.rt_denoise_guided(self.h, C.byref(p), *(abi.fptr(a) for a in planes), abi.fptr(variance), *out,
                                              abi.fptr(ov) if ov is not None else None), self._lib)
        return f, b, ov

    def denoise_guided_device(self, d_frame: int, d_albedo: int, d_normal: int, d_position: int, d_variance: int, d_out_f32: int = 0,
                              d_out_u8: int = 0, d_out_variance: int = 0, stream: int = 0, iterations: int = DENOISE_ITERATIONS, **params) -> None:
        """rt_denoise_guided_device on DEVICE pointers, enqueued on `stream`."""
        p = denoise_var_params(iterations, **params)
        v = [C.c_void_p(x or None) for x in (d_frame, d_albedo, d_normal, d_position, d_variance, d_out_f32, d_out_u8, d_out_variance, stream)]
        abi.check(self._lib.rt_denoise_guided_device(self.h, C.byref(p), *v), self._lib)

    def close(self):
        if self.h:
            self._lib.rt_denoiser_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# The temporal accumulator's defaults. sigma_position is TEMPORAL_POSITION_FRACTION of the scene's scale (Scene.scale()), as the
# denoiser's; host/main.cpp's --temporal uses the same values.
TEMPORAL_MAX_HISTORY = 32
TEMPORAL_POSITION_FRACTION = 0.05
TEMPORAL_COS_NORMAL = 0.9


def temporal_params(max_history: int = TEMPORAL_MAX_HISTORY, sigma_position: float | None = None, cos_normal: float = TEMPORAL_COS_NORMAL,
                    scene_scale: float | None = None):
    """rt_temporal_params; sigma_position None: TEMPORAL_POSITION_FRACTION * scene_scale, in fp32 (scene_scale is then required)."""
    sp = _sigma_position(sigma_position, TEMPORAL_POSITION_FRACTION, scene_scale, "sigma_position or scene_scale is required")
    return abi.rt_temporal_params(int(max_history), sp, float(cos_normal))


class TemporalAccumulator:
    """rt_temporal: temporal accumulation by reprojection for W x H frames on one device, guided by Scene.gbuffer_motion's planes. moments=True
    (RT_TEMPORAL_MOMENTS): the accumulator also carries the luminance moments that Denoiser.estimate_variance takes."""

    def __init__(self, device: int, width: int, height: int, lib=None, moments: bool = False):
        self._lib = lib or abi.load_library()
        self.width, self.height = int(width), int(height)
        self.moments = bool(moments)
        self.h = C.c_void_p()
        if moments:
            abi.check(self._lib.rt_temporal_create_ex(int(device), self.width, self.height, abi.RT_TEMPORAL_MOMENTS, C.byref(self.h)), self._lib)
        else:
            abi.check(self._lib.rt_temporal_create(int(device), self.width, self.height, C.byref(self.h)), self._lib)

    def accumulate(self, frame_f32: np.ndarray, gbuf: dict, camera: Camera, want_f32: bool = True, want_u8: bool = True,
                   out_f32: np.ndarray | None = None, moments: bool | None = None, **params):
        """rt_temporal_accumulate of a (H, W, 4) float32 frame rendered with `camera`, with the planes of Scene.gbuffer_motion(camera); returns
        (f32, u8, history_len (H, W) float32), None for an image not asked for. `params`: max_history, sigma_position, cos_normal, scene_scale
        (temporal_params). out_f32: where the fp32 result goes (may be frame_f32). On an accumulator created with moments=True the call is
        rt_temporal_accumulate_moments and the result a dict with the keys "f32", "u8", "history_len" and "moments" ((H, W, 2) float32);
        moments=False there makes the plain call (the accumulator keeps its moments up to date all the same)."""
        p = temporal_params(**params)
        shape = (self.height, self.width, 4)
        planes = _float_planes(shape, frame_f32, gbuf["normal"], gbuf["position"], gbuf["prev_position"])
        f, b, out = _outputs(shape, want_f32, want_u8, out_f32)
        n = np.zeros(shape[:2], np.float32)
        args = (self.h, C.byref(p), C.byref(camera.c), *(abi.fptr(a) for a in planes), *out, abi.fptr(n))
        if self.moments if moments is None else moments:
            m = np.zeros(shape[:2] + (2,), np.float32)
            abi.check(self._lib.rt_temporal_accumulate_moments(*args, abi.fptr(m)), self._lib)
            return {"f32": f, "u8": b, "history_len": n, "moments": m}
        abi.check(self._lib.rt_temporal_accumulate(*args), self._lib)
        return f, b, n

    def accumulate_device(self, camera: Camera, d_frame: int, d_normal: int, d_position: int, d_prev_position: int, d_out_f32: int = 0,
                          d_out_u8: int = 0, d_history_len: int = 0, stream: int = 0, **params) -> None:
        """rt_temporal_accumulate_device on DEVICE pointers (e.g. torch .data_ptr()), enqueued on `stream`."""
        p = temporal_params(**params)
        v = [C.c_void_p(x or None) for x in (d_frame, d_normal, d_position, d_prev_position, d_out_f32, d_out_u8, d_history_len, stream)]
        abi.check(self._lib.rt_temporal_accumulate_device(self.h, C.byref(p), C.byref(camera.c), *v), self._lib)

    def accumulate_moments_device(self, camera: Camera, d_frame: int, d_normal: int, d_position: int, d_prev_position: int, d_moments: int,
                                  d_out_f32: int = 0, d_out_u8: int = 0, d_history_len: int = 0, stream: int = 0, **params) -> None:
        """rt_temporal_accumulate_moments_device on DEVICE pointers, enqueued on `stream`."""
        p = temporal_params(**params)
        v = [C.c_void_p(x or None) for x in (d_frame, d_normal, d_position, d_prev_position, d_out_f32, d_out_u8, d_history_len, d_moments, stream)]
        abi.check(self._lib.rt_temporal_accumulate_moments_device(self.h, C.byref(p), C.byref(camera.c), *v), self._lib)

    def reset(self) -> None:
        """rt_temporal_reset: forget the history; the next call passes its frame through."""
        abi.check(self._lib.rt_temporal_reset(self.h), self._lib)

    def close(self):
        if self.h:
            self._lib.rt_temporal_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def assemble_tiles(parts: list[np.ndarray], height: int, world: int, strip_rows: int = 8) -> np.ndarray:
    """De-interleaves per-rank compact strip buffers (rank order) into the full frame."""
    w, ch = parts[0].shape[1], parts[0].shape[2]
    out = np.zeros((height, w, ch), parts[0].dtype)
    for rank, p in enumerate(parts):
        rows = [y for y in range(height) if (y // strip_rows) % world == rank]
        out[rows] = p[: len(rows)]
    return out
