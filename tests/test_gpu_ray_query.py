"""Ray queries with a per-ray tmax on the GPU (include/rt_mi355x.h: rt_trace_rays[_device], k_query<ANY> in rt_query.hip), bit for bit
against rt_intersect_batch and the CPU oracle's brute force. A hit counts iff 1e-4 < t <= tmax, so with the oracle's closest hit (t_h,
tri_h): CLOSEST = that hit where t_h <= tmax and a miss elsewhere, ANY = (tri_h != miss and t_h <= tmax)."""
import numpy as np
import pytest

from rtamd import abi, scenes
from rtamd.renderer import Scene

pytestmark = pytest.mark.gpu
NO_TRI = 0xFFFFFFFF
BVHS = [abi.RT_BVH_LBVH, abi.RT_BVH_SAH, abi.RT_BVH_LBVH_GPU]
SCENES = [("cornell", {}), ("atrium", {"detail": 1}), ("tables", {}), ("atrium_tilted", {"detail": 1})]


@pytest.fixture(scope="module")
def gpu(rtlib):
    assert rtlib.rt_device_count() > 0, "GPU tests need a device; the product has no CPU fallback"
    return 0


def parity_mix(sd, n, seed=5):
    """tests/test_gpu_parity.py's ray mix: random origins around the scene, unnormalised half-rounded directions, a third of the rays
    starting on triangle surfaces, axis-aligned directions with exact zeros."""
    rng = np.random.default_rng(seed)
    tw = sd.world_triangles()
    lo, hi = tw.reshape(-1, 3).min(0), tw.reshape(-1, 3).max(0)
    org = rng.uniform(lo - 0.1 * (hi - lo) - 0.5, hi + 0.1 * (hi - lo) + 0.5, (n, 3)).astype(np.float32)
    dirs = rng.normal(size=(n, 3)).astype(np.float32)
    dirs[: n // 4] *= 1e-2
    dirs = dirs.astype(np.float16).astype(np.float32)
    k = n // 3
    ti = rng.integers(0, sd.n_triangles, k)
    b = rng.dirichlet((1, 1, 1), k)
    org[:k] = np.einsum("ij,ijk->ik", b, tw[ti]).astype(np.float32)
    dirs[k: k + 60] = np.tile(np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [0, 1, 1], [-1, 0, 1], [1, 1, 0]], np.float32), (10, 1))
    return org, dirs


_ORACLE = {}


def oracle_mix(oracle, scene_cache, name, kw):
    """(org, dirs, (t, u, v, tri)) of the mix and the oracle's brute force, once per scene"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _ORACLE:
        sd = scene_cache(name, **kw)
        org, dirs = parity_mix(sd, 6000 if sd.n_triangles > 5000 else 20000)
        _ORACLE[key] = (org, dirs, oracle.OracleScene(sd).intersect(org, dirs, use_bvh=False))
    return _ORACLE[key]


def expected(closest, tmax):
    """CLOSEST and ANY with tmax from the closest hit without one"""
    t, u, v, tri = closest
    keep = (tri != NO_TRI) & (t <= tmax)
    f0 = np.float32(0)
    return (np.where(keep, t, np.float32(np.inf)), np.where(keep, u, f0), np.where(keep, v, f0), np.where(keep, tri, np.uint32(NO_TRI)),
            keep.astype(np.uint8))


def assert_closest(got, exp, what):
    for k, g, e in zip("t u v tri".split(), got, exp):
        np.testing.assert_array_equal(g, e, err_msg=f"{what}: {k}")


def trace_dev(s, org, dirs, tmax=None, any_hit=False, stream=None):
    """rt_trace_rays_device on torch tensors; returns numpy results"""
    import torch
    n = len(org)
    o, d = torch.from_numpy(np.ascontiguousarray(org)).cuda(), torch.from_numpy(np.ascontiguousarray(dirs)).cuda()
    tm = torch.from_numpy(np.ascontiguousarray(tmax, np.float32)).cuda() if tmax is not None else None
    st = stream or torch.cuda.current_stream()
    torch.cuda.synchronize()
    if any_hit:
        occ = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        s.trace_device(n, o.data_ptr(), d.data_ptr(), d_tmax=tm.data_ptr() if tm is not None else 0, d_occluded=occ.data_ptr(), any_hit=True,
                       stream=st.cuda_stream)
        st.synchronize()
        return occ.cpu().numpy()
    t, u, v = (torch.full((n,), 7.0, dtype=torch.float32, device="cuda") for _ in range(3))
    tri = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    s.trace_device(n, o.data_ptr(), d.data_ptr(), d_tmax=tm.data_ptr() if tm is not None else 0, d_t=t.data_ptr(), d_u=u.data_ptr(),
                   d_v=v.data_ptr(), d_tri=tri.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    return t.cpu().numpy(), u.cpu().numpy(), v.cpu().numpy(), tri.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name,kw", SCENES)
@pytest.mark.parametrize("bvh", BVHS)
def test_closest_without_tmax_equals_intersect_batch_and_the_oracle(gpu, oracle, scene_cache, name, kw, bvh):
    sd = scene_cache(name, **kw)
    org, dirs, e = oracle_mix(oracle, scene_cache, name, kw)
    s = Scene(sd, device=gpu, bvh=bvh)
    assert (e[3] != NO_TRI).sum() > len(org) // 50
    ib = s.intersect(org, dirs)
    assert_closest(ib, e, f"{name} rt_intersect_batch")
    assert_closest(s.trace(org, dirs), e, f"{name} rt_trace_rays")
    assert_closest(trace_dev(s, org, dirs), e, f"{name} rt_trace_rays_device")
    np.testing.assert_array_equal(s.trace(org, dirs, any_hit=True), (e[3] != NO_TRI).astype(np.uint8))
    np.testing.assert_array_equal(trace_dev(s, org, dirs, any_hit=True), (e[3] != NO_TRI).astype(np.uint8))
    s.close()


@pytest.mark.parametrize("name,kw", SCENES)
@pytest.mark.parametrize("bvh", [abi.RT_BVH_SAH, abi.RT_BVH_LBVH_GPU])
def test_tmax_edges(gpu, oracle, scene_cache, name, kw, bvh):
    """tmax = t_h counts, nextafter(t_h, 0) does not; tmax <= 1e-4, 0 and negative find nothing; random tmax in (0, 2 t_h)."""
    sd = scene_cache(name, **kw)
    org, dirs, e = oracle_mix(oracle, scene_cache, name, kw)
    s = Scene(sd, device=gpu, bvh=bvh)
    t_h = e[0]
    hit = e[3] != NO_TRI
    n = len(org)
    rng = np.random.default_rng(17)
    finite_t = np.where(hit, t_h, np.float32(1.0))
    cases = {
        "t_h": np.where(hit, t_h, np.float32(np.inf)).astype(np.float32),
        "below t_h": np.nextafter(finite_t, np.float32(0)).astype(np.float32),
        "tnear": np.full(n, np.float32(1e-4)),
        "zero": np.zeros(n, np.float32),
        "negative": np.full(n, np.float32(-1.0)),
        "-inf": np.full(n, -np.inf, np.float32),
        "random": (rng.uniform(0, 2, n) * finite_t).astype(np.float32),
    }
    for what, tmax in cases.items():
        ex = expected(e, tmax)
        assert_closest(s.trace(org, dirs, tmax), ex[:4], f"{name} {what}")
        np.testing.assert_array_equal(s.trace(org, dirs, tmax, any_hit=True), ex[4], err_msg=f"{name} {what}")
        np.testing.assert_array_equal(trace_dev(s, org, dirs, tmax, any_hit=True), ex[4], err_msg=f"{name} {what} device")
    assert expected(e, cases["t_h"])[4].sum() == hit.sum()
    assert expected(e, cases["below t_h"])[4].sum() == 0
    assert 0 < expected(e, cases["random"])[4].sum() < hit.sum()
    s.close()


def test_rejections(gpu, scene_cache):
    """Origins just inside and just outside the contract range (a few ulp either side of the limit on every axis and side), NaN and
    infinite origins, NaN tmax: the device marks exactly the rays the host entry refuses, which names the first of them."""
    sd = scene_cache("cube")
    s = Scene(sd, device=gpu)
    info = s.info()
    lo, hi = np.array(info.bounds_lo, np.float32), np.array(info.bounds_hi, np.float32)
    scale = np.float32(0)
    for a in range(3):
        scale = max(scale, max(np.float32(hi[a] - lo[a]), max(abs(lo[a]), abs(hi[a]))))
    limit = np.float32(100) * scale
    c = (lo + hi) / np.float32(2)
    org, tmax = [], []
    for a in range(3):
        for side in (-1, 1):
            edge = np.float32(hi[a] + limit) if side > 0 else np.float32(lo[a] - limit)
            x = edge
            for _ in range(4):
                x = np.nextafter(x, np.float32(-side * np.inf))
            for _ in range(9):  # 4 ulp inside ... 4 ulp outside
                o = c.copy()
                o[a] = x
                org.append(o), tmax.append(np.float32(np.inf))
                x = np.nextafter(x, np.float32(side * np.inf))
    for bad in (np.nan, np.inf, -np.inf):
        for a in range(3):
            o = c.copy()
            o[a] = bad
            org.append(o), tmax.append(np.float32(np.inf))
    for tm in (np.nan, 1.0, -np.nan):
        org.append(c.copy()), tmax.append(np.float32(tm))
    org = np.array(org, np.float32)
    tmax = np.array(tmax, np.float32)
    rng = np.random.default_rng(2)
    perm = rng.permutation(len(org))
    org, tmax = org[perm], tmax[perm]
    dirs = np.where(np.isfinite(org).all(1, keepdims=True), c - org + rng.normal(scale=0.1, size=org.shape), 1.0).astype(np.float32)
    refused = []
    for i in range(len(org)):
        try:
            s.trace(org[i: i + 1], dirs[i: i + 1], tmax[i: i + 1])
            refused.append(False)
        except abi.RtError as err:
            assert err.status == abi.RT_ERR_INVALID
            refused.append(True)
    refused = np.array(refused)
    assert 12 < refused.sum() < len(org) - 12  # both sides of the limit are there
    with pytest.raises(abi.RtError) as err:
        s.trace(org, dirs, tmax)
    assert f"ray {int(np.argmax(refused))}:" in str(err.value)
    t, u, v, tri = trace_dev(s, org, dirs, tmax)
    occ = trace_dev(s, org, dirs, tmax, any_hit=True)
    np.testing.assert_array_equal(tri == abi.RT_TRI_REJECTED, refused)
    np.testing.assert_array_equal(np.isnan(t), refused)
    np.testing.assert_array_equal(occ == 2, refused)
    assert (u[refused] == 7.0).all() and (v[refused] == 7.0).all()  # not written
    ok = ~refused
    e = s.intersect(org[ok], dirs[ok])
    ex = expected(e, tmax[ok])
    assert_closest((t[ok], u[ok], v[ok], tri[ok]), ex[:4], "accepted rays")
    np.testing.assert_array_equal(occ[ok], ex[4])
    s.close()


def _big_mix(sd, n):
    org, dirs = parity_mix(sd, n, seed=23)
    return org, dirs


@pytest.mark.parametrize("n", [1, 63, (1 << 22) + 17])
def test_sizes(gpu, scene_cache, n):
    sd = scene_cache("atrium")
    s = Scene(sd, device=gpu)
    org, dirs = _big_mix(sd, max(n, 1000))
    org, dirs = org[:n], dirs[:n]
    e = s.intersect(org, dirs)
    assert_closest(s.trace(org, dirs), e, f"n={n} host")
    assert_closest(trace_dev(s, org, dirs), e, f"n={n} device")
    rng = np.random.default_rng(n)
    tmax = np.where(rng.random(n) < 0.5, np.float32(1e-3), np.float32(np.inf)).astype(np.float32)  # short and unbounded rays side by side
    ex = expected(e, tmax)
    assert_closest(trace_dev(s, org, dirs, tmax), ex[:4], f"n={n} half short")
    np.testing.assert_array_equal(trace_dev(s, org, dirs, tmax, any_hit=True), ex[4])
    np.testing.assert_array_equal(s.trace(org, dirs, tmax, any_hit=True), ex[4])
    if n > 1000:
        assert ex[4].sum() < (e[3] != NO_TRI).sum()
    s.close()


@pytest.mark.parametrize("grid", [1, 3])
def test_the_persistent_regime_refills_every_wave_many_times(gpu, devlib, oracle, scene_cache, monkeypatch, grid):
    """RT_QUERY_GRID (developer library only) caps the persistent grid of both kernels. With one workgroup eight waves share 5,000 rays of
    the mix (32 shards of three chunks): every wave refills beside live lanes many times, and drains at the end. Both modes, without a tmax and with short,
    exact, random and unbounded ones side by side, against the oracle's brute force and against rt_intersect_batch."""
    monkeypatch.setenv("RT_QUERY_GRID", str(grid))
    sd = scene_cache("atrium", detail=1)
    org, dirs, e = oracle_mix(oracle, scene_cache, "atrium", {"detail": 1})
    n = 5000
    org, dirs, e = org[:n], dirs[:n], tuple(a[:n] for a in e)
    s = Scene(sd, device=gpu, lib=devlib)
    assert_closest(s.intersect(org, dirs), e, f"grid {grid} rt_intersect_batch")
    assert_closest(trace_dev(s, org, dirs), e, f"grid {grid}")
    np.testing.assert_array_equal(trace_dev(s, org, dirs, any_hit=True), (e[3] != NO_TRI).astype(np.uint8))
    rng = np.random.default_rng(grid)
    hit = e[3] != NO_TRI
    finite_t = np.where(hit, e[0], np.float32(1.0))
    kind = rng.integers(0, 4, n)
    tmax = np.select([kind == 0, kind == 1, kind == 2], [np.float32(1e-3), finite_t, rng.uniform(0, 2, n) * finite_t], np.inf).astype(np.float32)
    ex = expected(e, tmax)
    assert 0 < ex[4].sum() < hit.sum()
    assert_closest(trace_dev(s, org, dirs, tmax), ex[:4], f"grid {grid}, tmax mix")
    np.testing.assert_array_equal(trace_dev(s, org, dirs, tmax, any_hit=True), ex[4])
    assert_closest(s.trace(org, dirs, tmax), ex[:4], f"grid {grid}, tmax mix, host form")
    s.close()


def test_torch_stream_and_null_outputs(gpu, scene_cache):
    """Tensors on a non-default stream; outputs passed as NULL, and those of the other mode, are not written."""
    import torch
    sd = scene_cache("cornell")
    s = Scene(sd, device=gpu)
    org, dirs = parity_mix(sd, 5000, seed=8)
    n = len(org)
    rng = np.random.default_rng(4)
    tmax_h = (rng.uniform(0, 3, n) * np.float32(np.abs(org).max() + 1)).astype(np.float32)
    e = s.intersect(org, dirs)
    ex = expected(e, tmax_h)
    st = torch.cuda.Stream(device=0)
    o, d, tm = (torch.from_numpy(a).cuda() for a in (org, dirs, tmax_h))
    t = torch.full((n,), 5.0, dtype=torch.float32, device="cuda")
    u = torch.full((n,), 5.0, dtype=torch.float32, device="cuda")
    v = torch.full((n,), 5.0, dtype=torch.float32, device="cuda")
    tri = torch.full((n,), 5, dtype=torch.int32, device="cuda")
    occ = torch.full((n,), 5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        s.trace_device(n, o.data_ptr(), d.data_ptr(), d_tmax=tm.data_ptr(), d_t=t.data_ptr(), d_tri=tri.data_ptr(), d_occluded=occ.data_ptr(),
                       stream=st.cuda_stream)
    st.synchronize()
    np.testing.assert_array_equal(t.cpu().numpy(), ex[0])
    np.testing.assert_array_equal(tri.cpu().numpy().view(np.uint32), ex[3])
    assert (u.cpu().numpy() == 5.0).all() and (v.cpu().numpy() == 5.0).all() and (occ.cpu().numpy() == 5).all()
    t2 = torch.full((n,), 5.0, dtype=torch.float32, device="cuda")
    s.trace_device(n, o.data_ptr(), d.data_ptr(), d_tmax=tm.data_ptr(), d_t=t2.data_ptr(), d_occluded=occ.data_ptr(), any_hit=True,
                   stream=st.cuda_stream)
    st.synchronize()
    np.testing.assert_array_equal(occ.cpu().numpy(), ex[4])
    assert (t2.cpu().numpy() == 5.0).all()
    # two streams back to back share the scene's cursor: the later launch waits for the earlier one on the device
    st2 = torch.cuda.Stream(device=0)
    occ2 = torch.full((n,), 5, dtype=torch.uint8, device="cuda")
    with torch.cuda.stream(st):
        torch.cuda._sleep(50_000_000)
    s.trace_device(n, o.data_ptr(), d.data_ptr(), d_t=t.data_ptr(), d_tri=tri.data_ptr(), stream=st.cuda_stream)
    s.trace_device(n, o.data_ptr(), d.data_ptr(), d_tmax=tm.data_ptr(), d_occluded=occ2.data_ptr(), any_hit=True, stream=st2.cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(t.cpu().numpy(), e[0])
    np.testing.assert_array_equal(tri.cpu().numpy().view(np.uint32), e[3])
    np.testing.assert_array_equal(occ2.cpu().numpy(), ex[4])
    s.close()


def test_update_waits_for_pending_queries(gpu, scene_cache):
    """A query enqueued behind a long kernel, then rt_scene_update: the query answers for the old geometry; afterwards queries equal a
    fresh build of the moved scene."""
    import torch
    from test_scene_update import spin_about_centre
    sd = scene_cache("atrium")
    s = Scene(sd, device=gpu, updatable=True)
    org, dirs = parity_mix(sd, 200000, seed=9)
    n = len(org)
    before = s.intersect(org, dirs)
    tmax_h = np.full(n, np.float32(2.0))
    st = torch.cuda.Stream(device=0)
    o, d, tm = (torch.from_numpy(a).cuda() for a in (org, dirs, tmax_h))
    t, u, v = (torch.zeros(n, dtype=torch.float32, device="cuda") for _ in range(3))
    tri = torch.zeros(n, dtype=torch.int32, device="cuda")
    occ = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        torch.cuda._sleep(200_000_000)  # ~0.1 s of spinning in front of the queries
    s.trace_device(n, o.data_ptr(), d.data_ptr(), d_t=t.data_ptr(), d_u=u.data_ptr(), d_v=v.data_ptr(), d_tri=tri.data_ptr(), stream=st.cuda_stream)
    s.trace_device(n, o.data_ptr(), d.data_ptr(), d_tmax=tm.data_ptr(), d_occluded=occ.data_ptr(), any_hit=True, stream=st.cuda_stream)
    s.update(instances=spin_about_centre(sd, 25.0))
    torch.cuda.synchronize()
    assert_closest((t.cpu().numpy(), u.cpu().numpy(), v.cpu().numpy(), tri.cpu().numpy().view(np.uint32)), before, "pending query")
    np.testing.assert_array_equal(occ.cpu().numpy(), expected(before, tmax_h)[4])
    fresh = Scene(s.desc, device=gpu)
    moved = fresh.intersect(org, dirs)
    assert not np.array_equal(moved[3], before[3])  # the update did move the scene
    assert_closest(s.trace(org, dirs), moved, "after the update")
    assert_closest(trace_dev(s, org, dirs, tmax_h), expected(moved, tmax_h)[:4], "after the update, device")
    np.testing.assert_array_equal(trace_dev(s, org, dirs, tmax_h, any_hit=True), fresh.trace(org, dirs, tmax_h, any_hit=True))
    fresh.close(), s.close()


def test_empty_scene(gpu):
    s = Scene(scenes.get_scene("empty"), device=gpu)
    rng = np.random.default_rng(1)
    org = rng.normal(size=(1000, 3)).astype(np.float32)
    dirs = rng.normal(size=(1000, 3)).astype(np.float32)
    t, u, v, tri = s.trace(org, dirs)
    assert (t == np.inf).all() and (u == 0).all() and (v == 0).all() and (tri == NO_TRI).all()
    assert (s.trace(org, dirs, any_hit=True) == 0).all()
    assert (trace_dev(s, org, dirs, np.full(1000, np.float32(5)), any_hit=True) == 0).all()
    assert (trace_dev(s, org, dirs)[3] == NO_TRI).all()
    s.close()
