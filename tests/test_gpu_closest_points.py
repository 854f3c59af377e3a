"""Closest-point queries on the GPU (include/rt_mi355x.h: rt_closest_points[_device], k_closest in rt_closest.hip), bit for bit against
the host brute force rt_scene_closest_host(use_bvh = 0) — the contract's one text compiled for the host — and, on the Cornell box, against
the numpy model of tests/test_closest_points.py directly."""
import numpy as np
import pytest

from rtamd import abi, bake, scenes
from closest_scenes import radius_mix
from rtamd.renderer import ProbeVolume, Scene
from test_closest_points import NO_TRI, OUTPUTS, bounds_of, closest_model, point_mix, same, tri_scene, world_vertices

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def gpu(rtlib):
    assert rtlib.rt_device_count() > 0, "GPU tests need a device; the product has no CPU fallback"
    return 0


def closest_dev(s, pos, max_dist2=None, stream=None, outputs=OUTPUTS, canary=7):
    """rt_closest_points_device on torch tensors; returns numpy results (outputs not asked for keep the canary)"""
    import torch
    n = len(pos)
    p = torch.from_numpy(np.ascontiguousarray(pos, f32)).cuda()
    md = torch.from_numpy(np.ascontiguousarray(max_dist2, f32)).cuda() if max_dist2 is not None else None
    st = stream or torch.cuda.current_stream()
    bufs = {k: torch.full((n, 3) if k == "point" else (n,), canary, dtype=torch.int32 if k == "tri" else torch.float32, device="cuda")
            for k in OUTPUTS}
    torch.cuda.synchronize()
    s.closest_points_device(n, p.data_ptr(), d_max_dist2=md.data_ptr() if md is not None else 0, stream=st.cuda_stream,
                            **{"d_" + k: bufs[k].data_ptr() for k in outputs})
    st.synchronize()
    out = {k: bufs[k].cpu().numpy() for k in OUTPUTS}
    out["tri"] = out["tri"].view(np.uint32)
    return out


def host_form(s, pos, max_dist2=None):
    """rt_closest_points on host arrays with SQUARED radii (the wrapper Scene.closest_points squares a radius)"""
    import ctypes as C
    pos = np.ascontiguousarray(pos, f32)
    n = len(pos)
    out = {"dist2": np.zeros(n, f32), "u": np.zeros(n, f32), "v": np.zeros(n, f32), "tri": np.zeros(n, np.uint32), "point": np.zeros((n, 3), f32)}
    q = abi.rt_point_query(n=n, pos=pos.ctypes.data)
    if max_dist2 is not None:
        md = np.ascontiguousarray(max_dist2, f32)
        q.max_dist2 = md.ctypes.data
    for k, a in out.items():
        setattr(q, k, a.ctypes.data)
    abi.check(s._lib.rt_closest_points(s.h, C.byref(q)), s._lib)
    return out


def test_cornell_equals_the_model_and_the_host_brute_force_at_every_size(gpu, scene_cache):
    """n = 1, 63, 64, 65 and 513 (one lane, a wave less one, a wave, a wave and one, a workgroup and one) and 2,000, device and host forms,
    against closest_model directly and against rt_scene_closest_host(use_bvh = 0), with and without a radius mix."""
    sd = scene_cache("cornell")
    wv = world_vertices(sd)
    s = Scene(sd, device=gpu)
    pos_all = point_mix(sd, 2000, 31)
    for n in (1, 63, 64, 65, 513, 2000):
        pos = pos_all[:n]
        want = closest_model(pos, wv)
        same(s.closest_host(pos), want, f"n={n} host brute force vs model")
        same(closest_dev(s, pos), want, f"n={n} device")
        same(host_form(s, pos), want, f"n={n} host form")
        md2 = radius_mix(want["dist2"], n)
        want_r = closest_model(pos, wv, md2)
        same(closest_dev(s, pos, md2), want_r, f"n={n} device, radii")
        same(host_form(s, pos, md2), want_r, f"n={n} host form, radii")
    hit = want_r["tri"] != NO_TRI
    assert 0.5 < hit.mean() < 0.9  # the exact-boundary radii count, the ones just below do not
    out = s.closest_points(pos_all[:100], max_dist=1e6)
    np.testing.assert_array_equal(out["dist2"], want["dist2"][:100])
    np.testing.assert_array_equal(out["dist"], np.sqrt(want["dist2"][:100]))
    s.close()


@pytest.mark.parametrize("grid", [1, 3])
def test_the_persistent_regime_refills_every_wave_many_times(gpu, devlib, scene_cache, monkeypatch, grid):
    """RT_CLOSEST_GRID (developer library only) caps the persistent grid. With one workgroup eight waves share 5,000 points: every wave
    refills beside live lanes many times, and drains at the end."""
    monkeypatch.setenv("RT_CLOSEST_GRID", str(grid))
    sd = scene_cache("atrium", detail=1)
    s = Scene(sd, device=gpu, lib=devlib)
    pos = point_mix(sd, 5000, 41)
    want = s.closest_host(pos)
    same(closest_dev(s, pos), want, f"grid {grid}")
    md2 = radius_mix(want["dist2"], 2)
    same(closest_dev(s, pos, md2), s.closest_host(pos, md2), f"grid {grid}, radii")
    s.close()


def test_empty_scene_and_single_triangle(gpu, scene_cache):
    s = Scene(scenes.get_scene("empty"), device=gpu)
    pos = np.random.default_rng(1).normal(size=(1000, 3)).astype(f32)
    for out in (closest_dev(s, pos), host_form(s, pos), closest_dev(s, pos, np.full(1000, 5.0, f32))):
        assert np.isinf(out["dist2"]).all() and (out["dist2"] > 0).all() and (out["tri"] == NO_TRI).all()
        assert (out["u"] == 0).all() and (out["v"] == 0).all() and np.isnan(out["point"]).all()
    same(closest_dev(s, pos), s.closest_host(pos), "empty")
    s.close()
    sd = scene_cache("triangle")
    s = Scene(sd, device=gpu)
    pos = point_mix(sd, 2000, 6)
    want = closest_model(pos, world_vertices(sd))
    same(closest_dev(s, pos), want, "triangle")
    assert (want["tri"] == 0).all() and len(np.unique(np.stack([want["u"], want["v"]], 1), axis=0)) > 500  # every region is reached
    s.close()


@pytest.mark.parametrize("bvh", [abi.RT_BVH_SAH, abi.RT_BVH_LBVH_GPU])
def test_atrium_with_a_radius_mix(gpu, scene_cache, bvh):
    """Atrium at detail 1, the SAH build and the device-built LBVH: 4,096 points, no radius and a per-entry mix that includes radii exactly
    on the answer and one float below it."""
    sd = scene_cache("atrium", detail=1)
    s = Scene(sd, device=gpu, bvh=bvh)
    pos = point_mix(sd, 4096, 51)
    want = s.closest_host(pos)
    same(closest_dev(s, pos), want, "no radius")
    assert (want["tri"] != NO_TRI).all()
    md2 = radius_mix(want["dist2"], 9)
    want_r = s.closest_host(pos, md2)
    same(closest_dev(s, pos, md2), want_r, "radius mix")
    hit = want_r["tri"] != NO_TRI
    exact = md2 == want["dist2"]
    assert hit[exact & (md2 >= 0)].all() and exact.sum() > 500 and (~hit).sum() > 500
    _, _, scale = bounds_of(sd)
    r = f32(0.01 * scale)
    md2 = np.full(len(pos), r * r, f32)
    same(closest_dev(s, pos, md2), s.closest_host(pos, md2), "1 % radius")
    s.close()


def test_an_updated_scene_equals_a_fresh_build(gpu, scene_cache):
    from test_scene_update import spin_about_centre
    sd = scene_cache("atrium", detail=1)
    s = Scene(sd, device=gpu, updatable=True)
    pos = point_mix(sd, 4096, 61)
    before = closest_dev(s, pos)
    same(before, s.closest_host(pos), "before the update")
    s.update(instances=spin_about_centre(sd, 25.0))
    fresh = Scene(s.desc, device=gpu)
    want = fresh.closest_host(pos)
    assert not np.array_equal(want["tri"], before["tri"])  # the update did move the scene
    same(closest_dev(s, pos), want, "after the update, device")
    same(host_form(s, pos), want, "after the update, host form")
    same(s.closest_host(pos, use_bvh=True), want, "after the update, the host walk of the synchronised copy")
    same(closest_dev(fresh, pos), want, "fresh build")
    fresh.close(), s.close()


def test_rejected_entries_are_marked_and_the_rest_answered(gpu, scene_cache):
    """Points a few ulp either side of the contract range on every axis and side, NaN and infinite coordinates, NaN radii: the device marks
    exactly the entries the host form refuses, which names the first of them and writes nothing."""
    sd = scene_cache("cube")
    s = Scene(sd, device=gpu)
    info = s.info()
    lo, hi = np.array(info.bounds_lo, f32), np.array(info.bounds_hi, f32)
    scale = f32(max(max(f32(hi[a] - lo[a]), abs(lo[a]), abs(hi[a])) for a in range(3)))
    limit = f32(100) * scale
    c = (lo + hi) / f32(2)
    pos, md2 = [], []
    for a in range(3):
        for side in (-1, 1):
            x = f32(hi[a] + limit) if side > 0 else f32(lo[a] - limit)
            for _ in range(4):
                x = np.nextafter(x, f32(-side * np.inf))
            for _ in range(9):  # 4 ulp inside ... 4 ulp outside
                o = c.copy()
                o[a] = x
                pos.append(o), md2.append(f32(np.inf))
                x = np.nextafter(x, f32(side * np.inf))
    for bad in (np.nan, np.inf, -np.inf):
        for a in range(3):
            o = c.copy()
            o[a] = bad
            pos.append(o), md2.append(f32(np.inf))
    for m in (np.nan, 1.0, -np.nan, -1.0):
        pos.append(c.copy()), md2.append(f32(m))
    g = np.random.default_rng(2)
    perm = g.permutation(len(pos))
    pos, md2 = np.array(pos, f32)[perm], np.array(md2, f32)[perm]
    refused = []
    for i in range(len(pos)):
        try:
            host_form(s, pos[i: i + 1], md2[i: i + 1])
            refused.append(False)
        except abi.RtError as err:
            assert err.status == abi.RT_ERR_INVALID
            refused.append(True)
    refused = np.array(refused)
    assert 12 < refused.sum() < len(pos) - 12  # both sides of the limit are there
    with pytest.raises(abi.RtError) as err:
        host_form(s, pos, md2)
    assert f"point {int(np.argmax(refused))}:" in str(err.value)
    out = closest_dev(s, pos, md2)
    np.testing.assert_array_equal(out["tri"] == abi.RT_TRI_REJECTED, refused)
    np.testing.assert_array_equal(np.isnan(out["dist2"]), refused)
    assert (out["u"][refused] == 7.0).all() and (out["v"][refused] == 7.0).all() and (out["point"][refused] == 7.0).all()  # not written
    ok = ~refused
    want = s.closest_host(pos[ok], md2[ok])
    same({k: out[k][ok] for k in OUTPUTS}, want, "accepted entries")
    s.close()


def test_null_outputs_are_not_written(gpu, scene_cache):
    sd = scene_cache("cornell")
    s = Scene(sd, device=gpu)
    pos = point_mix(sd, 1000, 71)
    want = s.closest_host(pos)
    for asked in (("dist2",), ("tri",), ("point",), ("u", "v"), ("dist2", "tri", "point")):
        out = closest_dev(s, pos, outputs=asked, canary=5)
        for k in OUTPUTS:
            if k in asked:
                np.testing.assert_array_equal(out[k].view(np.uint32), want[k].view(np.uint32), err_msg=k)
            else:
                assert (out[k] == 5).all(), f"{k} was written though NULL"
    s.close()


def test_a_point_query_and_a_ray_query_on_two_streams_without_host_synchronisation(gpu, scene_cache):
    """The two launches share the scene's cursors: the later waits for the earlier on the device. Nothing synchronises between the
    enqueues; one synchronisation at the end."""
    import torch
    from test_gpu_ray_query import parity_mix
    sd = scene_cache("atrium", detail=1)
    s = Scene(sd, device=gpu)
    pos = point_mix(sd, 8192, 81)
    org, dirs = parity_mix(sd, 8192, seed=3)
    n = len(pos)
    want_p, want_r = s.closest_host(pos), s.intersect(org, dirs)
    st1, st2 = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    p, o, d = (torch.from_numpy(a).cuda() for a in (pos, org, dirs))
    d2 = torch.full((n,), 5.0, dtype=torch.float32, device="cuda")
    ptri = torch.full((n,), 5, dtype=torch.int32, device="cuda")
    t = torch.full((n,), 5.0, dtype=torch.float32, device="cuda")
    rtri = torch.full((n,), 5, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(3):
        s.closest_points_device(n, p.data_ptr(), d_dist2=d2.data_ptr(), d_tri=ptri.data_ptr(), stream=st1.cuda_stream)
        s.trace_device(n, o.data_ptr(), d.data_ptr(), d_t=t.data_ptr(), d_tri=rtri.data_ptr(), stream=st2.cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d2.cpu().numpy().view(np.uint32), want_p["dist2"].view(np.uint32))
    np.testing.assert_array_equal(ptri.cpu().numpy().view(np.uint32), want_p["tri"])
    np.testing.assert_array_equal(t.cpu().numpy(), want_r[0])
    np.testing.assert_array_equal(rtri.cpu().numpy().view(np.uint32), want_r[3])
    s.close()


def test_distance_grid_is_the_clearance_of_a_probe_volumes_probes(gpu, scene_cache):
    sd = scene_cache("cornell")
    s = Scene(sd, device=gpu)
    origin, count = bake.probe_grid(sd, 0.5, margin=0.1)
    vol = ProbeVolume(s, origin, 0.5, count, max_dirs=4)
    dist, tri = bake.distance_grid(s, vol.origin, vol.spacing, vol.count)
    assert dist.shape == tuple(vol.count[::-1]) and tri.shape == dist.shape
    want = s.closest_host(vol.positions())
    np.testing.assert_array_equal(dist.reshape(-1), np.sqrt(want["dist2"]))
    np.testing.assert_array_equal(tri.reshape(-1), want["tri"])
    r = f32(np.median(dist))
    near, tri_r = bake.distance_grid(s, vol.origin, vol.spacing, vol.count, max_dist=r)
    inside = want["dist2"] <= r * r
    np.testing.assert_array_equal(tri_r.reshape(-1) != NO_TRI, inside)
    assert inside.any() and (~inside).any() and np.isinf(near.reshape(-1)[~inside]).all()
    vol.close(), s.close()
